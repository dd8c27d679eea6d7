// guidance_test.cpp — the host residue map (guidance_where) and the host agreement counts (msa_agreement_host) of host/guidance.cpp
// on hand-made alignments: all gaps, one residue per column, identical replicates (the maximum N * (occ - 1)), disjoint replicates
// (zero), a shifted replicate, rows that do not hold the same residues (refused), the bounds of one call and the exact newick text.
// Linked with guidance.cpp and the driver's own parallel_for (host_threads.cpp: the pooled threads, so that a sanitizer sees the rows
// being counted concurrently); built by tests/test_cpu_guidance.py with -fsanitize=address,undefined from this file, those two,
// phytree.cpp and alphabet.cpp.
// Prints "ok <checks>" and exits 0, or says what differs.
#include "pgm_host.h"

#include <algorithm>
#include <cstdio>
#include <sstream>

using namespace pgm;

static int checks = 0, failures = 0;
static void expect(const char *what, bool ok) {
    ++checks;
    if (!ok) { ++failures; printf("FAIL %s\n", what); }
}

static std::vector<sequence_t> rows_of(const std::vector<std::string> &text) {
    std::vector<sequence_t> out;
    for (const std::string &s : text) out.emplace_back(s.begin(), s.end());
    return out;
}

struct Counts { std::vector<uint32_t> res, pair; };
// the counts of `base` against the replicates `reps`, output buffers pre-filled with garbage
static Counts count(const Alphabet &a, const std::vector<std::string> &base, const std::vector<std::vector<std::string>> &reps, std::vector<int32_t> *where_out = nullptr) {
    const size_t n = base.size(), L = base[0].size();
    std::vector<int32_t> where(reps.size() * n * L, 12345);
    for (size_t r = 0; r < reps.size(); ++r) guidance_where(a, rows_of(base), rows_of(reps[r]), where.data() + r * n * L);
    Counts c;
    c.res.assign(n * L, 0xdeadbeefu);
    c.pair.assign(n * n, 0xdeadbeefu);
    msa_agreement_host((uint32_t)n, (uint32_t)L, (uint32_t)reps.size(), where.data(), c.res.data(), c.pair.data());
    if (where_out) *where_out = where;
    return c;
}
static bool all_zero(const std::vector<uint32_t> &v) { return std::all_of(v.begin(), v.end(), [](uint32_t x) { return x == 0; }); }

int main() {
    const Alphabet a(ALPHA_AA);
    {   // all gaps: every entry of where is -1, nothing hits
        const std::vector<std::string> base = {"----", "----", "----"};
        std::vector<int32_t> where;
        const Counts c = count(a, base, {{"--", "--", "--"}, {"-----", "-----", "-----"}}, &where);
        expect("all gaps: where", std::all_of(where.begin(), where.end(), [](int32_t w) { return w == -1; }));
        expect("all gaps: counts", all_zero(c.res) && all_zero(c.pair));
    }
    {   // one residue per column: no column holds a pair, whatever the replicates do
        const std::vector<std::string> base = {"A--", "-C-", "--D"};
        const Counts c = count(a, base, {{"A", "C", "D"}, {"A--", "-C-", "--D"}, {"-A", "C-", "D-"}});
        expect("one residue per column: residues", all_zero(c.res));
        // (the first and third replicates put residues of different base columns into one column: those are no base pairs)
        expect("one residue per column: pairs", all_zero(c.pair));
    }
    {   // identical replicates: every residue meets its occ - 1 column mates in each of the N replicates
        const std::vector<std::string> base = {"AC-DE", "A-CDE", "-CCD-", "A---E"};
        const uint32_t occ[5] = {3, 2, 2, 3, 3}, N = 5;
        std::vector<int32_t> where;
        const Counts c = count(a, base, std::vector<std::vector<std::string>>(N, base), &where);
        bool ok = true, map_ok = true;
        for (size_t i = 0; i < 4; ++i)
            for (size_t col = 0; col < 5; ++col) {
                ok = ok && c.res[i * 5 + col] == (base[i][col] == '-' ? 0u : N * (occ[col] - 1));
                for (uint32_t r = 0; r < N; ++r) map_ok = map_ok && where[(r * 4 + i) * 5 + col] == (base[i][col] == '-' ? -1 : (int32_t)col);
            }
        expect("identical replicates: where", map_ok);
        expect("identical replicates: residues at the maximum", ok);
        bool pok = true;
        for (size_t i = 0; i < 4; ++i)
            for (size_t j = 0; j < 4; ++j) {
                uint32_t both = 0;
                for (size_t col = 0; col < 5; ++col) both += base[i][col] != '-' && base[j][col] != '-';
                pok = pok && c.pair[i * 4 + j] == (i == j ? 0u : N * both) && c.pair[i * 4 + j] == c.pair[j * 4 + i];
            }
        expect("identical replicates: pairs", pok);
    }
    {   // disjoint replicates: every row in columns of its own
        const std::vector<std::string> base = {"ACD", "ACD", "ACD"};
        const std::vector<std::string> rep = {"ACD------", "---ACD---", "------ACD"};
        const Counts c = count(a, base, {rep, rep});
        expect("disjoint replicates", all_zero(c.res) && all_zero(c.pair));
    }
    {   // a shifted replicate: row 1 moved by one column keeps nothing with row 0; rows 0 and 2 keep all three columns
        const std::vector<std::string> base = {"ACD", "ACD", "ACD"};
        std::vector<int32_t> where;
        const Counts c = count(a, base, {{"ACD-", "-ACD", "ACD-"}}, &where);
        const std::vector<int32_t> want_where = {0, 1, 2, 1, 2, 3, 0, 1, 2};
        expect("shifted: where", where == want_where);
        const std::vector<uint32_t> want_res = {1, 1, 1, 0, 0, 0, 1, 1, 1}, want_pair = {0, 0, 3, 0, 0, 0, 3, 0, 0};
        expect("shifted: residues", c.res == want_res);
        expect("shifted: pairs", c.pair == want_pair);
    }
    {   // rows that do not hold the same number of residues are refused
        int thrown = 0;
        std::vector<int32_t> where(6);
        try { guidance_where(a, rows_of({"ACD", "AC-"}), rows_of({"AC", "AC"}), where.data()); } catch (pgm_exception &) { ++thrown; }
        try { guidance_where(a, rows_of({"AC-", "AC-"}), rows_of({"ACD", "AC-"}), where.data()); } catch (pgm_exception &) { ++thrown; }
        try { guidance_where(a, rows_of({"AC-", "AC-"}), rows_of({"AC", "AC", "AC"}), where.data()); } catch (pgm_exception &) { ++thrown; }
        expect("unequal rows refused", thrown == 3);
    }
    {   // codon symbols: the gap is the alphabet's own value, not '-'
        const Alphabet ca(ALPHA_CODON);
        const sequence_t b0 = {0, ca.gap(), 5}, b1 = {ca.gap(), 7, 9};
        const sequence_t r0 = {ca.gap(), 0, 5}, r1 = {7, ca.gap(), 9};
        std::vector<int32_t> where(6);
        guidance_where(ca, {b0, b1}, {r0, r1}, where.data());
        const std::vector<int32_t> want = {1, -1, 2, -1, 0, 2};
        expect("codon where", where == want);
    }
    {   // the bounds of one call
        expect("call bound: bytes", guidance_call_replicates(10, 10, 4000) == 10 && guidance_call_replicates(10, 10, 399) == 1);
        expect("call bound: columns", (uint64_t)guidance_call_replicates(2, 3000000000u, (size_t)1 << 62) * 3000000000ull <= 0xffffffffull);
        expect("call bound: rows", guidance_call_replicates(70000, 1, (size_t)1 << 62) == 0xffffffffull / 69999);
        int thrown = 0;
        try { msa_agreement_host(3, 0x80000000u, 2, nullptr, nullptr, nullptr); } catch (pgm_exception &) { ++thrown; }
        expect("host counts refuse sums beyond 32 bits", thrown == 1);
    }
    {   // %.17g round trip
        PhyTree root, *x = new PhyTree("x"), *y = new PhyTree("y"), *in = new PhyTree(), *z = new PhyTree("z");
        in->addChild(x, 0.1); in->addChild(y, 1.0 / 3.0);
        root.addChild(in, 2e-9); root.addChild(z, 7);
        expect("exact newick", format_newick_exact(root) == "((x:0.10000000000000001,y:0.33333333333333331):2.0000000000000001e-09,z:7);");
    }
    if (failures) { printf("%d of %d checks failed\n", failures, checks); return 1; }
    printf("ok %d\n", checks);
    return 0;
}
