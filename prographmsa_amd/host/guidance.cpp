// guidance.cpp — the host parts of `pgmsa --guidance` that need no driver state: the residue map
// between the base alignment and a replicate alignment, the host statement of the agreement counts (Backend::msa_agreement's
// default, what pgmsa_oracle runs), the bounds of one agreement call, the exact newick text of a replicate's guide tree and the
// two score files.  The flow that joins them (bootstrap trees, forest passes, groups) is doGuidance in driver_analyses.cpp.
#include "pgm_host.h"

#include <algorithm>
#include <cstdio>
#include <ostream>

namespace pgm {

GuidanceStats guidance_stats;

// where[i * ncols + c] for one replicate: row i keeps its residues in their order, so its k-th residue stands in the base's
// k-th non-gap column and in the replicate's k-th non-gap column
void guidance_where(const Alphabet &a, const std::vector<sequence_t> &base, const std::vector<sequence_t> &rep, int32_t *where) {
    if (base.size() != rep.size()) error("guidance: a replicate alignment of %zu rows for a base alignment of %zu", rep.size(), base.size());
    const size_t ncols = base.empty() ? 0 : base[0].size();
    for (size_t i = 0; i < base.size(); ++i) {
        if (base[i].size() != ncols) error("guidance: rows of different length in the base alignment");
        if (rep[i].size() != rep[0].size()) error("guidance: rows of different length in a replicate alignment");
        if (rep[i].size() > 0x7fffffffull) error("guidance: a replicate alignment of %zu columns", rep[i].size());
        int32_t *w = where + i * ncols;
        size_t p = 0;
        for (size_t c = 0; c < ncols; ++c) {
            if (a.isGap(base[i][c])) { w[c] = -1; continue; }
            while (p < rep[i].size() && a.isGap(rep[i][p])) ++p;
            if (p == rep[i].size()) error("guidance: row %zu has fewer residues in a replicate alignment than in the base alignment", i);
            w[c] = (int32_t)p++;
        }
        while (p < rep[i].size() && a.isGap(rep[i][p])) ++p;
        if (p != rep[i].size()) error("guidance: row %zu has more residues in a replicate alignment than in the base alignment", i);
    }
}

void msa_agreement_host(uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where, uint32_t *res_hits, uint32_t *pair_hits) {
    if ((uint64_t)nrep * (nrows ? nrows - 1 : 0) > 0xffffffffull || (uint64_t)nrep * ncols > 0xffffffffull)
        error("msa agreement: nrep * (nrows - 1) or nrep * ncols does not fit 32 bits");
    parallel_for(nrows, [&](size_t i) {
        uint32_t *res = res_hits + i * ncols, *pair = pair_hits + i * nrows;
        std::fill(res, res + ncols, 0u);
        std::fill(pair, pair + nrows, 0u);
        for (uint32_t r = 0; r < nrep; ++r) {
            const int32_t *rep = where + (size_t)r * nrows * ncols, *wi = rep + i * ncols;
            for (uint32_t j = 0; j < nrows; ++j) {
                if (j == i) continue;
                const int32_t *wj = rep + (size_t)j * ncols;
                uint32_t n = 0;
                for (uint32_t c = 0; c < ncols; ++c) {
                    const uint32_t hit = (wi[c] >= 0 && wi[c] == wj[c]) ? 1u : 0u;   // (two gaps never hit)
                    res[c] += hit;
                    n += hit;
                }
                pair[j] += n;
            }
        }
    });
}

void Backend::msa_agreement(uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where, uint32_t *res_hits, uint32_t *pair_hits, int) {
    msa_agreement_host(nrows, ncols, nrep, where, res_hits, pair_hits);
}

uint32_t guidance_call_replicates(uint32_t nrows, uint32_t ncols, size_t where_bytes) {
    uint64_t m = where_bytes / std::max<uint64_t>(1, sizeof(int32_t) * (uint64_t)nrows * ncols);
    if (nrows > 1) m = std::min<uint64_t>(m, 0xffffffffull / (nrows - 1));
    if (ncols > 0) m = std::min<uint64_t>(m, 0xffffffffull / ncols);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(m, 0xffffffffull));
}

static void newick_exact(const PhyTree &t, std::string &s) {
    if (t.isLeaf()) { s += t.getName(); return; }
    s += '(';
    for (index_t i = 0; i < t.n_children(); ++i) {
        if (i) s += ',';
        newick_exact(t[(int)i], s);
        char buf[40];
        snprintf(buf, sizeof buf, ":%.17g", t[(int)i].getBranchLength());
        s += buf;
    }
    s += ')';
}
std::string format_newick_exact(const PhyTree &tree) {
    std::string s;
    newick_exact(tree, s);
    return s + ";";
}

namespace {
void guidance_line(std::ostream &out, uint64_t hits, uint64_t pairs) {
    char buf[96];
    if (pairs) snprintf(buf, sizeof buf, "%llu\t%llu\t%.6f\n", (unsigned long long)hits, (unsigned long long)pairs, (double)hits / (double)pairs);
    else snprintf(buf, sizeof buf, "%llu\t%llu\tNA\n", (unsigned long long)hits, (unsigned long long)pairs);
    out << buf;
}
}  // namespace

void guidance_write(const GuidanceCounts &g, const std::vector<std::string> &names, const int32_t *where0, uint64_t seed, std::ostream &out, std::ostream *residues) {
    const size_t n = g.nrows, L = g.ncols;
    const uint64_t N = g.nrep;
    std::vector<uint64_t> occ(L, 0);
    for (size_t i = 0; i < n; ++i)
        for (size_t c = 0; c < L; ++c) occ[c] += where0[i * L + c] >= 0 ? 1u : 0u;
    out << "# guidance replicates=" << N << " seed=" << seed << " sequences=" << n << " columns=" << L << "\n";
    std::vector<uint64_t> chits(L, 0), cpairs(L, 0);
    uint64_t ahits = 0, apairs = 0;
    for (size_t c = 0; c < L; ++c) {
        for (size_t i = 0; i < n; ++i) chits[c] += g.res_hits[i * L + c];
        chits[c] /= 2;
        cpairs[c] = occ[c] ? N * (occ[c] * (occ[c] - 1) / 2) : 0;
        ahits += chits[c]; apairs += cpairs[c];
    }
    out << "alignment\t"; guidance_line(out, ahits, apairs);
    for (size_t c = 0; c < L; ++c) { out << "column\t" << (c + 1) << "\t"; guidance_line(out, chits[c], cpairs[c]); }
    for (size_t i = 0; i < n; ++i) {
        uint64_t hits = 0, pairs = 0;
        for (size_t c = 0; c < L; ++c) {
            hits += g.res_hits[i * L + c];
            if (where0[i * L + c] >= 0) pairs += N * (occ[c] - 1);
        }
        out << "sequence\t" << names[i] << "\t"; guidance_line(out, hits, pairs);
    }
    std::vector<uint64_t> both(n * n, 0);   // columns in which both rows hold a residue
    parallel_for(n, [&](size_t i) {
        for (size_t j = i + 1; j < n; ++j) {
            uint64_t b = 0;
            for (size_t c = 0; c < L; ++c) b += (where0[i * L + c] >= 0 && where0[j * L + c] >= 0) ? 1u : 0u;
            both[i * n + j] = b;
        }
    });
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j) { out << "pair\t" << names[i] << "\t" << names[j] << "\t"; guidance_line(out, g.pair_hits[i * n + j], N * both[i * n + j]); }
    if (residues)
        for (size_t i = 0; i < n; ++i)
            for (size_t c = 0; c < L; ++c)
                if (where0[i * L + c] >= 0) { *residues << names[i] << "\t" << (c + 1) << "\t"; guidance_line(*residues, g.res_hits[i * L + c], N * (occ[c] - 1)); }
}

}  // namespace pgm
