// bootstrap_test.cpp — bipartition_support (host/phytree.cpp) on hand-written trees of 4 to 7 leaves: exact counts, printed the way
// --bootstrap_out prints them (PhyTree::formatNewick with labels).  Leaf 0 is "a" (sorted-name order).  Built by
// tests/test_cpu_bootstrap.py from this file, phytree.cpp and alphabet.cpp; prints "ok <checks>" and exits 0, or says what differs.
#include "pgm_host.h"

#include <cstdio>
#include <memory>
#include <sstream>

using namespace pgm;

static int checks = 0, failures = 0;

static PhyTree *tree_of(const std::string &newick) {
    std::istringstream in(newick);
    return parse_newick(in);
}

// the labelled text of `tree` with the replicates `reps` (each `times` times)
static std::string labelled(const std::string &tree, const std::vector<std::pair<std::string, int>> &reps) {
    std::unique_ptr<PhyTree> t(tree_of(tree));
    std::vector<std::unique_ptr<PhyTree>> own;
    std::vector<const PhyTree *> r;
    for (const auto &p : reps)
        for (int k = 0; k < p.second; ++k) { own.emplace_back(tree_of(p.first)); r.push_back(own.back().get()); }
    return t->formatNewick(bipartition_support(*t, r));
}

static void expect(const char *what, const std::string &got, const std::string &want) {
    ++checks;
    if (got != want) { ++failures; printf("FAIL %s\n  got  %s\n  want %s\n", what, got.c_str(), want.c_str()); }
}

int main() {
    // 6 leaves: ab | cdef (the two root edges), cd, ef
    const std::string T6 = "((a:1,b:1):1,((c:1,d:1):1,(e:1,f:1):1):1);";
    // without labels the text is formatNewick()'s
    {
        std::unique_ptr<PhyTree> t(tree_of(T6));
        expect("plain text", t->formatNewick(std::map<const PhyTree *, uint32_t>()), t->formatNewick());
        expect("round trip", t->formatNewick(), T6);
    }
    // identical trees: N everywhere, the two root edges the same number
    expect("identical x5", labelled(T6, {{T6, 5}}), "((a:1,b:1)5:1,((c:1,d:1)5:1,(e:1,f:1)5:1)5:1);");
    expect("no replicates", labelled(T6, {}), "((a:1,b:1)0:1,((c:1,d:1)0:1,(e:1,f:1)0:1)0:1);");
    // one replicate is one NNI away (d and (e,f) swapped around the edge cd | abef): N - 1 on exactly that edge
    const std::string T6_nni = "((a:1,b:1):1,((c:1,(e:1,f:1):1):1,d:1):1);";
    expect("one NNI", labelled(T6, {{T6, 4}, {T6_nni, 1}}), "((a:1,b:1)5:1,((c:1,d:1)4:1,(e:1,f:1)5:1)5:1);");
    // an NNI around the root edge (b and (c,d) swapped): both root edges lose the replicate, the same number on both
    const std::string T6_nni_root = "((a:1,(c:1,d:1):1):1,(b:1,(e:1,f:1):1):1);";
    expect("NNI at the root edge", labelled(T6, {{T6, 2}, {T6_nni_root, 1}}), "((a:1,b:1)2:1,((c:1,d:1)3:1,(e:1,f:1)3:1)2:1);");
    // the same topology rooted elsewhere (on the branch of c), and unrooted with three children at the root: no change
    const std::string T6_on_c = "(c:1,(d:1,((e:1,f:1):1,(a:1,b:1):1):1):1);", T6_unrooted = "((a:1,b:1):1,(c:1,d:1):1,(e:1,f:1):1);";
    expect("other rootings", labelled(T6, {{T6_on_c, 2}, {T6_unrooted, 3}, {T6, 1}}), "((a:1,b:1)6:1,((c:1,d:1)6:1,(e:1,f:1)6:1)6:1);");
    // ... and the other way round: the tree rooted on a leaf's branch (its internal root child cuts off c alone: no label)
    expect("rooted on a leaf", labelled(T6_on_c, {{T6, 2}, {T6_nni, 1}}), "(c:1,(d:1,((e:1,f:1)3:1,(a:1,b:1)3:1)2:1):1);");
    expect("three root children", labelled(T6_unrooted, {{T6, 2}, {T6_nni, 1}}), "((a:1,b:1)3:1,(c:1,d:1)2:1,(e:1,f:1)3:1);");
    // leaf 0 on either side: the clade with a first or last, a deep inside it; 7 leaves: ab, abc | defg, de, fg
    const std::string T7 = "(((a:1,b:1):1,c:1):1,((d:1,e:1):1,(f:1,g:1):1):1);", T7_flipped = "((f:1,g:1):1,((d:1,e:1):1,(c:1,(b:1,a:1):1):1):1);";
    expect("leaf 0 first", labelled(T7, {{T7_flipped, 3}}), "(((a:1,b:1)3:1,c:1)3:1,((d:1,e:1)3:1,(f:1,g:1)3:1)3:1);");
    expect("leaf 0 last", labelled(T7_flipped, {{T7, 3}}), "((f:1,g:1)3:1,((d:1,e:1)3:1,(c:1,(b:1,a:1)3:1)3:1)3:1);");
    // (c and the clade de swapped: abc | defg and ab stay, de stays, abde... : only the edge abc | defg goes)
    const std::string T7_other = "(((a:1,b:1):1,(d:1,e:1):1):1,(c:1,(f:1,g:1):1):1);";
    expect("leaf 0, another topology", labelled(T7, {{T7_flipped, 2}, {T7_other, 2}}), "(((a:1,b:1)4:1,c:1)2:1,((d:1,e:1)4:1,(f:1,g:1)4:1)2:1);");
    // 4 and 5 leaves
    expect("4 leaves", labelled("((a:1,b:1):1,(c:1,d:1):1);", {{"((a:1,b:1):1,(c:1,d:1):1);", 2}, {"((a:1,c:1):1,(b:1,d:1):1);", 1}, {"(a:1,(b:1,(c:1,d:1):1):1);", 1}}),
           "((a:1,b:1)3:1,(c:1,d:1)3:1);");
    expect("5 leaves", labelled("((a:1,b:1):1,((c:1,d:1):1,e:1):1);", {{"(e:1,((a:1,b:1):1,(c:1,d:1):1):1);", 2}, {"((a:1,e:1):1,((c:1,d:1):1,b:1):1);", 1}}),
           "((a:1,b:1)2:1,((c:1,d:1)3:1,e:1)2:1);");
    // a replicate over other leaves is an error, not a count
    ++checks;
    try { labelled(T6, {{T7, 1}}); ++failures; printf("FAIL a replicate with other leaves was accepted\n"); }
    catch (std::exception &) {}
    if (failures) { printf("%d of %d checks failed\n", failures, checks); return 1; }
    printf("ok %d\n", checks);
    return 0;
}
