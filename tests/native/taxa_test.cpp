// taxa_test.cpp — transfer_taxa_host and taxa_support (host/transfer.cpp) on hand-written trees of 8 and 9 leaves and on hand-made
// sets: exact counts, and the two file texts the way --bootstrap_taxa prints them.  Leaf 0 is "a" (sorted-name order).
// Linked with transfer.cpp and the driver's own parallel_for (host_threads.cpp); built by tests/test_cpu_taxa.py with
// -fsanitize=address,undefined from this file, those two, phytree.cpp and alphabet.cpp.  Prints "ok <checks>" and exits 0, or says what differs.
#include "pgm_host.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <sstream>

using namespace pgm;

static int checks = 0, failures = 0;

// "((a,b),c)" -> "((a:1,b:1):1,c:1);": a branch of length 1 on every edge
static std::string nwk(const std::string &shape) {
    std::string s;
    for (char c : shape) {
        if (c == ',' || c == ')') s += ":1";
        s += c;
    }
    return s + ";";
}
static PhyTree *tree_of(const std::string &newick) {
    std::istringstream in(newick);
    return parse_newick(in);
}

static TaxaSupport support(const std::string &tree, const std::vector<std::pair<std::string, int>> &reps, double cutoff) {
    std::unique_ptr<PhyTree> t(tree_of(nwk(tree)));
    std::vector<std::unique_ptr<PhyTree>> own;
    std::vector<const PhyTree *> r;
    for (const auto &p : reps)
        for (int k = 0; k < p.second; ++k) { own.emplace_back(tree_of(nwk(p.first))); r.push_back(own.back().get()); }
    return taxa_support(*t, r, cutoff);
}

static void expect(const char *what, const std::string &got, const std::string &want) {
    ++checks;
    if (got != want) { ++failures; printf("FAIL %s\n  got  %s\n  want %s\n", what, got.c_str(), want.c_str()); }
}
static void expect_true(const char *what, bool ok) {
    ++checks;
    if (!ok) { ++failures; printf("FAIL %s\n", what); }
}
static void expect_prefix(const char *what, const std::string &got, const std::string &want) { expect(what, got.substr(0, want.size()), want); }
typedef std::vector<uint64_t> U64;

struct Taxa { std::vector<uint32_t> phi, arg, moved, counted; };
// transfer_taxa_host on one-word sets, every output pre-filled with garbage
static Taxa taxa_of(uint32_t n, const U64 &ref, const std::vector<uint32_t> &thr, const std::vector<U64> &reps) {
    U64 b;
    std::vector<uint32_t> off(1, 0);
    for (const auto &rep : reps) {
        b.insert(b.end(), rep.begin(), rep.end());
        off.push_back(off.back() + (uint32_t)rep.size());
    }
    Taxa t;
    t.phi.assign(ref.size() * reps.size(), 0xdeadbeefu);
    t.arg.assign(ref.size() * reps.size(), 0xdeadbeefu);
    t.moved.assign(ref.size() * n, 0xdeadbeefu);
    t.counted.assign(ref.size(), 0xdeadbeefu);
    transfer_taxa_host(n, (uint32_t)ref.size(), ref.data(), thr.data(), (uint32_t)reps.size(), off.data(), b.empty() ? nullptr : b.data(), t.phi.data(), t.arg.data(),
                       t.moved.data(), t.counted.data());
    return t;
}

int main() {
    const uint32_t NONE = kTransferNone;
    // 8 leaves: ab, cd, abcd | efgh (the two root edges: one bipartition), ef, gh
    const std::string T8 = "(((a,b),(c,d)),((e,f),(g,h)))";
    // identical replicates: nothing moves, every edge counted in every replicate; the shared root bipartition enters K once
    {
        const TaxaSupport s = support(T8, {{T8, 3}}, 0.3);
        expect("identical x3", taxa_text(s, 0.3),
               "# replicates 3 cutoff 0.3 edges 5 counted 15\ntaxon\tmoved\tscore\na\t0\t0.000000\nb\t0\t0.000000\nc\t0\t0.000000\nd\t0\t0.000000\n"
               "e\t0\t0.000000\nf\t0\t0.000000\ng\t0\t0.000000\nh\t0\t0.000000\n");
        expect("identical x3: edges", taxa_edges_text(s),
               "edge\tp\tcounted\ta\tb\tc\td\te\tf\tg\th\n0\t2\t3\t0\t0\t0\t0\t0\t0\t0\t0\n1\t2\t3\t0\t0\t0\t0\t0\t0\t0\t0\n2\t4\t3\t0\t0\t0\t0\t0\t0\t0\t0\n"
               "3\t2\t3\t0\t0\t0\t0\t0\t0\t0\t0\n4\t2\t3\t0\t0\t0\t0\t0\t0\t0\t0\n5\t4\t3\t0\t0\t0\t0\t0\t0\t0\t0\n");
        expect_true("identical: six labelled nodes, five bipartitions", s.nodes.size() == 6 && s.edges == 5 && s.counted == 15);
    }
    // a caterpillar whose leaf c sits beside h in every replicate: c is the one moved leaf on the edges between the two places.
    // cutoff 0.99: thr = floor(0.99 (p - 1)) = 0, 1, 2, 1, 0 for cdefgh, defgh, efgh, fgh, gh; gh has phi 1 = p - 1 (reached by
    // cgh, but above thr 0), so it is not counted
    {
        const std::string cat = "(a,(b,(c,(d,(e,(f,(g,h)))))))", cat_moved = "(a,(b,(d,(e,(f,(g,(h,c)))))))";
        const TaxaSupport s = support(cat, {{cat_moved, 4}}, 0.99);
        expect("caterpillar", taxa_text(s, 0.99),
               "# replicates 4 cutoff 0.99 edges 5 counted 16\ntaxon\tmoved\tscore\na\t0\t0.000000\nb\t0\t0.000000\nc\t12\t0.750000\nd\t0\t0.000000\n"
               "e\t0\t0.000000\nf\t0\t0.000000\ng\t0\t0.000000\nh\t0\t0.000000\n");
        // post-order: gh, fgh, efgh, defgh, cdefgh
        expect("caterpillar: edges", taxa_edges_text(s),
               "edge\tp\tcounted\ta\tb\tc\td\te\tf\tg\th\n0\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\n1\t3\t4\t0\t0\t4\t0\t0\t0\t0\t0\n2\t4\t4\t0\t0\t4\t0\t0\t0\t0\t0\n"
               "3\t3\t4\t0\t0\t4\t0\t0\t0\t0\t0\n4\t2\t4\t0\t0\t0\t0\t0\t0\t0\t0\n");
        // thr = 0 (cutoff 0): only the edge both trees have is counted, and nothing moves
        const TaxaSupport z = support(cat, {{cat_moved, 4}, {cat, 1}}, 0.0);
        expect_true("cutoff 0", z.counted == 4 + 5 && std::all_of(z.moved.begin(), z.moved.end(), [](uint64_t v) { return v == 0; }) && z.nodes[4].counted == 5 &&
                                    z.nodes[0].counted == 1);
        expect_prefix("cutoff 0: header", taxa_text(z, 0.0), "# replicates 5 cutoff 0 edges 5 counted 9\ntaxon\tmoved\tscore\na\t0\t0.000000\n");
    }
    // a forced tie, 9 leaves: the edge abcd | efghi is one leaf from abc (T = {d}) and one from abcde (T = {e}); on the side without
    // leaf a these are defghi = 0x1f8 and fghi = 0x1e0, so abcde is the canonically smaller and e is the moved leaf, however the
    // replicate stores the two
    {
        const std::string T9 = "(((a,b),(c,d)),((e,f),(g,(h,i))))";
        const std::vector<std::string> stored = {"((((a,b),c),(d,e)),(f,(g,h)),i)", "(i,((h,g),f),((e,d),(c,(b,a))))", "((d,e),((a,b),c),(i,(f,(g,h))))",
                                                 "(f,((g,h),(i,((e,d),((a,b),c)))))"};
        std::string first;
        for (const std::string &rep : stored) {
            const TaxaSupport s = support(T9, {{rep, 1}}, 0.5);
            // post-order: ab, cd, abcd, ef, hi, ghi, efghi; abcd and efghi are one bipartition
            expect_true("tie: the smaller set's leaf", s.nodes.size() == 7 && s.nodes[2].p == 4 && s.nodes[2].counted == 1 &&
                                                           s.nodes[2].moved == U64({0, 0, 0, 0, 1, 0, 0, 0, 0}) && s.nodes[6].moved == s.nodes[2].moved && s.edges == 6);
            const std::string text = taxa_text(s, 0.5) + taxa_edges_text(s);
            if (first.empty()) first = text;
            expect("tie: the same files for every stored order", text, first);
        }
    }
    // a replicate with no non-trivial set (a star): no arg-min, nothing counted; mixed with a real one
    {
        const TaxaSupport s = support(T8, {{"(a,b,c,d,e,f,g,h)", 2}}, 0.99);
        expect_true("star", s.counted == 0 && s.replicates == 2 && std::all_of(s.moved.begin(), s.moved.end(), [](uint64_t v) { return v == 0; }));
        expect_prefix("star: score 0 when K = 0", taxa_text(s, 0.99), "# replicates 2 cutoff 0.99 edges 5 counted 0\ntaxon\tmoved\tscore\na\t0\t0.000000\nb\t0\t0.000000\n");
        const TaxaSupport m = support(T8, {{"(a,b,c,d,e,f,g,h)", 2}, {T8, 1}}, 0.99);
        expect_true("star and tree", m.counted == 5 && m.nodes[0].counted == 1);
        expect_true("no replicates", support(T8, {}, 0.3).counted == 0 && support(T8, {}, 0.3).nodes.size() == 6);
    }

    // ---- transfer_taxa_host on sets: 8 leaves, bit k = leaf k ----
    {
        // both orientations of T: abcd against abcde (h = 1) and against its complement fgh (h = 7): leaf e either way
        const Taxa t = taxa_of(8, {0x0f}, {3}, {{0x1f}, {0xe0}, {0x1f, 0xe0}, {0xe0, 0x1f}});
        expect_true("orientations", t.phi == std::vector<uint32_t>({1, 1, 1, 1}) && t.arg == std::vector<uint32_t>({0, 1, 2, 4}) && t.counted[0] == 4 &&
                                        t.moved == std::vector<uint32_t>({0, 0, 0, 0, 4, 0, 0, 0}));
        // the lowest index among equal distances; a set twice; thr below phi; an empty replicate; a replicate only the clamp reaches
        // ab (p = 2, clamp 1): abc and abd are one leaf away (c, d), cdefgh is its complement (distance 0), efgh is two away
        const Taxa u = taxa_of(8, {0x03, 0x03}, {1, 0}, {{0x07, 0x0b}, {0x0b, 0x07}, {0x07, 0xfc, 0x03}, {}, {0xf0}, {0xf0, 0x07, 0x07}});
        expect_true("lowest index: phi", u.phi == std::vector<uint32_t>({1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1}));
        expect_true("lowest index: arg", u.arg == std::vector<uint32_t>({0, 2, 5, NONE, NONE, 9, 0, 2, 5, NONE, NONE, 9}));
        expect_true("lowest index: moved", u.moved == std::vector<uint32_t>({0, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}) && u.counted == std::vector<uint32_t>({4, 1}));
        // p = 1 (a single leaf): phi 0 by the clamp; counted only where a replicate has that very set
        const Taxa v = taxa_of(8, {0x01}, {0xffffffffu}, {{0x03}, {0xfe}, {}});
        expect_true("p = 1", v.phi == std::vector<uint32_t>({0, 0, 0}) && v.arg == std::vector<uint32_t>({NONE, 1, NONE}) && v.counted[0] == 1 &&
                                 std::all_of(v.moved.begin(), v.moved.end(), [](uint32_t x) { return x == 0; }));
        // 70 leaves, two words: A = leaves 0..34; B = leaves 0..33 and 69 (T = {34, 69}); C = the complement of A but for leaf 40 (T = {40})
        const uint64_t lo35 = ((uint64_t)1 << 35) - 1, lo34 = ((uint64_t)1 << 34) - 1;
        const U64 A = {lo35, 0}, BC = {lo34, 0x20, ~lo35 & ~((uint64_t)1 << 40), 0x3f};
        const uint32_t off[4] = {0, 1, 2, 2}, thr70[1] = {2};
        std::vector<uint32_t> phi(3, 7u), arg(3, 7u), moved(70, 7u), counted(1, 7u);
        transfer_taxa_host(70, 1, A.data(), thr70, 3, off, BC.data(), phi.data(), arg.data(), moved.data(), counted.data());
        std::vector<uint32_t> want(70, 0);
        want[34] = want[69] = want[40] = 1;
        expect_true("70 leaves", phi == std::vector<uint32_t>({2, 1, 34}) && arg == std::vector<uint32_t>({0, 1, NONE}) && moved == want && counted[0] == 2);
    }
    // what the contract rejects is an error, and the outputs stay as they were
    {
        std::vector<uint32_t> phi(2, 77u), arg(2, 77u), moved(16, 77u), counted(2, 77u);
        const uint64_t ref[2] = {0x03, 0x0c}, rep[1] = {0x30}, high[1] = {0x103}, full[1] = {0xff}, none[1] = {0};
        const uint32_t off[2] = {0, 1}, off_bad[2] = {1, 1}, off_desc[3] = {0, 1, 0}, thr[2] = {1, 1};
        int thrown = 0, tried = 0;
        auto refused = [&](const std::function<void()> &f) { ++tried; try { f(); } catch (pgm_exception &) { ++thrown; } };
        auto call = [&](uint32_t n, uint32_t nref, const uint64_t *rf, const uint32_t *th, uint32_t nrep, const uint32_t *of, const uint64_t *rp, int null_out = -1) {
            refused([&] {
                transfer_taxa_host(n, nref, rf, th, nrep, of, rp, null_out == 0 ? nullptr : phi.data(), null_out == 1 ? nullptr : arg.data(),
                                   null_out == 2 ? nullptr : moved.data(), null_out == 3 ? nullptr : counted.data());
            });
        };
        call(3, 2, ref, thr, 1, off, rep);
        call(8, 0, ref, thr, 1, off, rep);
        call(8, 2, ref, thr, 0, off, rep);
        call(8, 2, nullptr, thr, 1, off, rep);
        call(8, 2, ref, nullptr, 1, off, rep);
        call(8, 2, ref, thr, 1, nullptr, rep);
        call(8, 2, ref, thr, 1, off, nullptr);
        for (int k = 0; k < 4; ++k) call(8, 2, ref, thr, 1, off, rep, k);
        call(8, 2, ref, thr, 1, off_bad, rep);
        call(8, 1, ref, thr, 2, off_desc, rep);
        call(8, 1, high, thr, 1, off, rep);
        call(8, 2, ref, thr, 1, off, high);
        call(8, 1, full, thr, 1, off, rep);
        call(8, 1, none, thr, 1, off, rep);
        call(8, 0x10000u, ref, thr, 0x10000u, off, rep);        // nref * nrep beyond 32 bits
        call(0x10000u, 0x10000u, ref, thr, 1, off, rep);        // nref * nleaves beyond 32 bits
        call(0x80000000u, 1, ref, thr, 1, off, rep);            // nleaves beyond 2^31 - 1
        expect_true("every rejection throws", thrown == tried);
        auto untouched = [](const std::vector<uint32_t> &v) { return std::all_of(v.begin(), v.end(), [](uint32_t x) { return x == 77u; }); };
        expect_true("a refused call leaves the outputs alone", untouched(phi) && untouched(arg) && untouched(moved) && untouched(counted));
        ++checks;
        try { support(T8, {{T8, 1}}, 1.0); ++failures; printf("FAIL a cutoff of 1 was accepted\n"); }
        catch (pgm_exception &) {}
    }
    if (failures) { printf("%d of %d checks failed\n", failures, checks); return 1; }
    printf("ok %d\n", checks);
    return 0;
}
