// transfer_test.cpp — transfer_min_host and transfer_support (host/transfer.cpp) on hand-written trees of 5 to 8 leaves and on
// hand-made sets: exact transfer indices, printed the way --bootstrap_tbe prints them.  Leaf 0 is "a" (sorted-name order).
// Linked with transfer.cpp and the driver's own parallel_for (host_threads.cpp); built by tests/test_cpu_transfer.py with
// -fsanitize=address,undefined from this file, those two, phytree.cpp and alphabet.cpp.  Prints "ok <checks>" and exits 0, or says what differs.
#include "pgm_host.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <sstream>

using namespace pgm;

static int checks = 0, failures = 0;

// "((a,b)0.5,c)" -> "((a:1,b:1)0.5:1,c:1);": a branch of length 1 on every edge
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

struct Support { std::string text; std::vector<std::pair<uint64_t, uint32_t>> edges; };   // edges: (S, p) in the order of the labelled nodes' addresses
static Support support(const std::string &tree, const std::vector<std::pair<std::string, int>> &reps) {
    std::unique_ptr<PhyTree> t(tree_of(nwk(tree)));
    std::vector<std::unique_ptr<PhyTree>> own;
    std::vector<const PhyTree *> r;
    for (const auto &p : reps)
        for (int k = 0; k < p.second; ++k) { own.emplace_back(tree_of(nwk(p.first))); r.push_back(own.back().get()); }
    const auto sup = transfer_support(*t, r);
    Support out;
    out.text = t->formatNewick(transfer_labels(sup, (uint32_t)r.size()));
    for (const auto &kv : sup) out.edges.emplace_back(kv.second.S, kv.second.p);
    return out;
}

static void expect(const char *what, const std::string &got, const std::string &want) {
    ++checks;
    if (got != want) { ++failures; printf("FAIL %s\n  got  %s\n  want %s\n", what, got.c_str(), want.c_str()); }
}
static void expect_true(const char *what, bool ok) {
    ++checks;
    if (!ok) { ++failures; printf("FAIL %s\n", what); }
}

// phi of ref against the replicates `reps` (sets as words), the output pre-filled with garbage
static std::vector<uint32_t> phi_of(uint32_t n, const std::vector<std::vector<uint64_t>> &ref, const std::vector<std::vector<std::vector<uint64_t>>> &reps) {
    std::vector<uint64_t> r, b;
    std::vector<uint32_t> off(1, 0);
    for (const auto &s : ref) r.insert(r.end(), s.begin(), s.end());
    for (const auto &rep : reps) {
        for (const auto &s : rep) b.insert(b.end(), s.begin(), s.end());
        off.push_back(off.back() + (uint32_t)rep.size());
    }
    std::vector<uint32_t> phi(ref.size() * reps.size(), 0xdeadbeefu);
    transfer_min_host(n, (uint32_t)ref.size(), r.data(), (uint32_t)reps.size(), off.data(), b.empty() ? nullptr : b.data(), phi.data());
    return phi;
}

int main() {
    // 8 leaves: ab, cd, abcd | efgh (the two root edges), ef, gh
    const std::string T8 = "(((a,b),(c,d)),((e,f),(g,h)))";
    {
        std::unique_ptr<PhyTree> t(tree_of(nwk(T8)));
        expect("plain text", t->formatNewick(std::map<const PhyTree *, std::string>()), t->formatNewick());
        expect("round trip", t->formatNewick(), nwk(T8));
    }
    // an identical tree: every index 0, every label 1.000000
    {
        const Support s = support(T8, {{T8, 3}});
        expect("identical x3", s.text, nwk("(((a,b)1.000000,(c,d)1.000000)1.000000,((e,f)1.000000,(g,h)1.000000)1.000000)"));
        expect_true("identical: S == 0", s.edges.size() == 6 && std::all_of(s.edges.begin(), s.edges.end(), [](const std::pair<uint64_t, uint32_t> &e) { return e.first == 0; }));
    }
    // a star: only single-leaf edges, so every index is p - 1 and every label 0.000000
    const std::string star8 = "(a,b,c,d,e,f,g,h)";
    {
        const Support s = support(T8, {{star8, 2}});
        expect("star x2", s.text, nwk("(((a,b)0.000000,(c,d)0.000000)0.000000,((e,f)0.000000,(g,h)0.000000)0.000000)"));
        expect_true("star: S == N (p - 1)", std::all_of(s.edges.begin(), s.edges.end(), [](const std::pair<uint64_t, uint32_t> &e) { return e.first == 2ull * (e.second - 1); }));
    }
    // leaf c moved from beside d onto the branch above (e,f): index 1 on exactly the edges between the two places (cd, abcd | efgh)
    const std::string moved = "(((a,b),d),(((e,f),c),(g,h)))";
    expect("one leaf moved, N = 1", support(T8, {{moved, 1}}).text, nwk("(((a,b)1.000000,(c,d)0.000000)0.666667,((e,f)1.000000,(g,h)1.000000)0.666667)"));
    expect("one leaf moved, 1 of 4", support(T8, {{T8, 3}, {moved, 1}}).text,
           nwk("(((a,b)1.000000,(c,d)0.750000)0.916667,((e,f)1.000000,(g,h)1.000000)0.916667)"));
    // the same replicate rooted on the branch of g, and with three children at the root: the same values
    const std::string moved_on_g = "(g,(h,(((e,f),c),((a,b),d))))", moved_unrooted = "(((a,b),d),((e,f),c),(g,h))";
    expect("other rootings", support(T8, {{moved_on_g, 1}}).text, support(T8, {{moved, 1}}).text);
    expect("three root children", support(T8, {{moved_unrooted, 1}}).text, support(T8, {{moved, 1}}).text);
    expect("rootings mixed", support(T8, {{T8, 1}, {moved_on_g, 1}, {moved_unrooted, 1}, {T8, 1}}).text,
           nwk("(((a,b)1.000000,(c,d)0.500000)0.833333,((e,f)1.000000,(g,h)1.000000)0.833333)"));
    // the tree itself with three root children, and rooted on a leaf's branch (its internal root child cuts off g alone: no label)
    expect("tree with three root children", support("((a,b),(c,d),((e,f),(g,h)))", {{moved, 1}}).text,
           nwk("((a,b)1.000000,(c,d)0.000000,((e,f)1.000000,(g,h)1.000000)0.666667)"));
    expect("tree rooted on a leaf", support("(g,(h,((e,f),((a,b),(c,d)))))", {{moved_on_g, 1}}).text,
           nwk("(g,(h,((e,f)1.000000,((a,b)1.000000,(c,d)0.000000)0.666667)1.000000))"));
    // leaf 0 on either side: the clade with a first or last
    const std::string T7 = "(((a,b),c),((d,e),(f,g)))", T7_flipped = "((f,g),((d,e),(c,(b,a))))", T7_other = "(((a,b),(d,e)),(c,(f,g)))";
    expect("leaf 0 first", support(T7, {{T7_flipped, 3}}).text, nwk("(((a,b)1.000000,c)1.000000,((d,e)1.000000,(f,g)1.000000)1.000000)"));
    expect("leaf 0 last", support(T7_flipped, {{T7, 3}}).text, nwk("((f,g)1.000000,((d,e)1.000000,(c,(b,a)1.000000)1.000000)1.000000)"));
    // (c and the clade de swapped: abc | defg is one leaf away from abde | cfg, p = 3: 1 - 1 / 2)
    expect("another topology", support(T7, {{T7_other, 1}}).text, nwk("(((a,b)1.000000,c)0.500000,((d,e)1.000000,(f,g)1.000000)0.500000)"));
    // 5 leaves: ab | cde and cd | abe; the replicate has ae | bcd and cd
    expect("5 leaves", support("((a,b),((c,d),e))", {{"((a,e),((c,d),b))", 1}, {"((a,b),((c,d),e))", 1}}).text, nwk("((a,b)0.500000,((c,d)1.000000,e)0.500000)"));
    // no replicates, and a replicate over other leaves
    expect("no replicates", support(T8, {}).text, nwk(T8));
    ++checks;
    try { support(T8, {{T7, 1}}); ++failures; printf("FAIL a replicate with other leaves was accepted\n"); }
    catch (std::exception &) {}

    // ---- transfer_min_host on sets ----
    {
        // 8 leaves, bit k = leaf k: ab = 0x03, cd = 0x0c, abcd = 0x0f, ef = 0x30; replicates: the moved tree, none at all, the star
        const std::vector<std::vector<uint64_t>> ref = {{0x03}, {0x0c}, {0x0f}, {0x30}, {0x01}};   // (the last: p = 1, always 0)
        const std::vector<std::vector<uint64_t>> moved_sets = {{0x03}, {0x0b}, {0x30}, {0x34}, {0xc0}, {0xf4}};
        const std::vector<uint32_t> phi = phi_of(8, ref, {moved_sets, {}, moved_sets});
        expect_true("sets: moved / empty / moved", phi == std::vector<uint32_t>({0, 1, 0, 1, 1, 1, 1, 3, 1, 0, 1, 0, 0, 0, 0}));
        // every set on its other side: the same indices
        auto flip = [](std::vector<std::vector<uint64_t>> v) { for (auto &s : v) s[0] ^= 0xff; return v; };
        expect_true("sets: complemented", phi_of(8, flip(ref), {flip(moved_sets), {}, moved_sets}) == phi && phi_of(8, ref, {flip(moved_sets), {}, flip(moved_sets)}) == phi);
        // 70 leaves, two words: A = leaves 0..34, B = leaves 0..33 and 69 (two leaves apart), C = the complement of A but for leaf 40
        const uint64_t lo35 = ((uint64_t)1 << 35) - 1, lo34 = ((uint64_t)1 << 34) - 1;
        const std::vector<uint64_t> A = {lo35, 0}, B = {lo34, 0x20}, C = {~lo35 & ~((uint64_t)1 << 40), 0x3f};
        expect_true("sets: 70 leaves", phi_of(70, {A}, {{B}, {C}, {B, C}, {}}) == std::vector<uint32_t>({2, 1, 1, 34}));
    }
    // what the contract rejects is an error, and the output stays as it was
    {
        std::vector<uint32_t> phi(2, 77u);
        const uint64_t ref[2] = {0x03, 0x0c}, rep[1] = {0x30}, high[1] = {0x103}, full[1] = {0xff}, none[1] = {0};
        const uint32_t off[2] = {0, 1}, off_bad[2] = {1, 1}, off_desc[3] = {0, 1, 0};
        int thrown = 0, tried = 0;
        auto refused = [&](const std::function<void()> &f) { ++tried; try { f(); } catch (pgm_exception &) { ++thrown; } };
        refused([&] { transfer_min_host(3, 2, ref, 1, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 0, ref, 1, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 2, ref, 0, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 2, nullptr, 1, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 2, ref, 1, nullptr, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 2, ref, 1, off, nullptr, phi.data()); });
        refused([&] { transfer_min_host(8, 2, ref, 1, off, rep, nullptr); });
        refused([&] { transfer_min_host(8, 2, ref, 1, off_bad, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 1, ref, 2, off_desc, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 1, high, 1, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 2, ref, 1, off, high, phi.data()); });
        refused([&] { transfer_min_host(8, 1, full, 1, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 1, none, 1, off, rep, phi.data()); });
        refused([&] { transfer_min_host(8, 0x10000u, ref, 0x10000u, off, rep, phi.data()); });
        expect_true("every rejection throws", thrown == tried);
        expect_true("a refused call leaves phi alone", phi[0] == 77u && phi[1] == 77u);
    }
    // the bounds of one call
    expect_true("call bounds", transfer_call_replicates(1024, 1021, 1021, (size_t)1 << 30) == 8216 && transfer_call_replicates(70, 67, 67, 100) == 1 &&
                                   transfer_call_replicates(8, 0x80000000u, 5) == 1 && transfer_call_replicates(8, 5, 5, 80) == 2);
    if (failures) { printf("%d of %d checks failed\n", failures, checks); return 1; }
    printf("ok %d\n", checks);
    return 0;
}
