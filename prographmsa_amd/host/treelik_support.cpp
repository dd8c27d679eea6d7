// treelik_support.cpp — branch support on the ML tree for `pgmsa --ml_tree --ml_support` (it reads the candidates' scores of
// treelik_nni.cpp): the host statement of pgm_resampled_sums
// (Backend::resampled_sums's default, what pgmsa_oracle runs), and the aLRT, SH-like and RELL values of every supported node, which
// are host code and the same for every backend.
#include "pgm_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>

namespace pgm {

MlSupportStats ml_support_stats;

void resampled_sums_host(uint32_t nrow, uint32_t ncols, const double *x, uint32_t nrep, const uint32_t *cols, double *out) {
    if (!x || !cols || !out) error("resampled sums: null argument");
    if (nrow == 0 || ncols == 0 || nrep == 0) error("resampled sums: nrow, ncols and nrep must be at least 1");
    if ((uint64_t)nrow * nrep > 0xffffffffull) error("resampled sums: nrow * nrep = %llu does not fit 32 bits", (unsigned long long)nrow * nrep);
    if ((uint64_t)nrep * ncols > 0xffffffffull) error("resampled sums: nrep * ncols = %llu does not fit 32 bits", (unsigned long long)nrep * ncols);
    const size_t entries = (size_t)nrep * ncols;
    for (size_t k = 0; k < entries; ++k)
        if (cols[k] >= ncols) error("resampled sums: replicate %zu draws column %u of %u", k / ncols, cols[k], ncols);
    // rows x chunks of replicates on the host threads; every sum is one chain, k ascending from 0.0
    const size_t chunk = 64, nchunks = ((size_t)nrep + chunk - 1) / chunk;
    parallel_for((size_t)nrow * nchunks, [&](size_t item) {
        const size_t q = item / nchunks, r0 = item % nchunks * chunk, r1 = std::min<size_t>(nrep, r0 + chunk);
        const double *row = x + q * ncols;
        for (size_t r = r0; r < r1; ++r) {
            const uint32_t *c = cols + r * ncols;
            double acc = 0.0;
            for (uint32_t k = 0; k < ncols; ++k) acc = acc + row[c[k]];
            out[q * nrep + r] = acc;
        }
    });
}

void Backend::resampled_sums(uint32_t nrow, uint32_t ncols, const double *x, uint32_t nrep, const uint32_t *cols, double *out, int) {
    resampled_sums_host(nrow, ncols, x, nrep, cols, out);
}

void ml_support_candidates(uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, std::vector<uint32_t> &node, std::vector<uint32_t> &cand_v,
                           std::vector<uint32_t> &cand_a, std::vector<uint32_t> &cand_c) {
    node.clear(); cand_v.clear(); cand_a.clear(); cand_c.clear();
    if (nnodes == 0) return;
    std::vector<std::vector<uint32_t>> kids(nnodes);
    for (uint32_t v = 0; v + 1 < nnodes; ++v) kids[parent[v]].push_back(v);
    const uint32_t root = nnodes - 1;
    for (uint32_t v = nleaves; v + 1 < nnodes; ++v) {
        const uint32_t u = parent[v];
        if (u == root && kids[u].size() == 2) continue;   // (around a binary root the interchanges only move the root along one edge)
        node.push_back(v);
        for (uint32_t a : kids[v])
            for (uint32_t c : kids[u])
                if (c != v) { cand_v.push_back(v); cand_a.push_back(a); cand_c.push_back(c); }
    }
}

std::vector<MlSupportNode> ml_branch_support(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                             uint32_t ncat, const double *w, const double *P, uint32_t nrep, const uint32_t *cols, Backend *be, size_t x_bytes,
                                             const MlSupportOpt *opt) {
    const auto t0 = std::chrono::steady_clock::now();
    if (nrep == 0 || !cols) error("ml support: no replicate");
    std::vector<uint32_t> node, cv, ca, cc;
    ml_support_candidates(nleaves, nnodes, parent, node, cv, ca, cc);
    std::vector<MlSupportNode> out(node.size());
    ml_support_stats.nodes += node.size();
    if (node.empty()) {
        ml_support_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return out;
    }
    // the likelihood ratios of every candidate at every column, and their logarithms
    const uint32_t ncand = (uint32_t)cv.size();
    std::vector<double> site_l(ncols), post((size_t)ncat * ncols), x((size_t)ncand * ncols), gain(ncand);
    std::vector<int32_t> site_k(ncols);
    const double nni_ms = ml_search_stats.kernel_ms;   // (the search's key counts its own calls alone)
    if (opt && opt->rounds) {   // every neighbour at its own central length
        MlNniEdgeResult found = ml_nni_edge_lengths(*opt->mf, nleaves, nnodes, parent, ncols, rows, *opt->rates, P, *opt->lengths, ncand, cv.data(), ca.data(), cc.data(),
                                                    opt->rounds, be);
        x.swap(found.rho);
    } else if (be) be->tree_nni(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cv.data(), ca.data(), cc.data(), site_l.data(), site_k.data(), post.data(), x.data());
    else tree_nni_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cv.data(), ca.data(), cc.data(), site_l.data(), site_k.data(), post.data(), x.data());
    ml_support_stats.kernel_ms += ml_search_stats.kernel_ms - nni_ms;
    ml_search_stats.kernel_ms = nni_ms;
    treelik_nni_gain(ncand, ncols, x.data(), gain.data());
    for (double &v : x) v = std::log(v);   // (log 0 is -infinity)
    // the resampled gains, rows in groups whose x stays within x_bytes and whose sums fit 32 bits
    std::vector<double> D((size_t)ncand * nrep);
    const size_t per_call = std::max<size_t>(1, std::min<size_t>(x_bytes / (8 * (size_t)ncols), 0xffffffffull / nrep));
    for (size_t q0 = 0; q0 < ncand; q0 += per_call) {
        const uint32_t g = (uint32_t)std::min<size_t>(per_call, ncand - q0);
        if (be) be->resampled_sums(g, ncols, x.data() + q0 * ncols, nrep, cols, D.data() + q0 * nrep);
        else resampled_sums_host(g, ncols, x.data() + q0 * ncols, nrep, cols, D.data() + q0 * nrep);
        ++ml_support_stats.calls;
    }
    // the statistics per node
    size_t q = 0;
    for (size_t n = 0; n < node.size(); ++n) {
        MlSupportNode &s = out[n];
        s.node = node[n];
        std::vector<uint32_t> C;   // the candidates that are not infinitely worse
        for (; q < ncand && cv[q] == node[n]; ++q) {
            ++s.candidates;
            if (gain[q] != -INFINITY) C.push_back((uint32_t)q);
        }
        if (C.empty()) { s.alrt = INFINITY; s.sh_hits = s.rell_hits = nrep; continue; }
        double best = gain[C[0]];
        for (uint32_t c : C) best = gain[c] > best ? gain[c] : best;
        const double d_obs = -best;
        s.alrt = 2.0 * d_obs;
        std::vector<double> mean(C.size());
        for (size_t j = 0; j < C.size(); ++j) {
            double acc = 0.0;
            for (uint32_t r = 0; r < nrep; ++r) acc = acc + D[(size_t)C[j] * nrep + r];
            mean[j] = acc / (double)nrep;
        }
        for (uint32_t r = 0; r < nrep; ++r) {
            double top = 0.0, second = -INFINITY;   // (e_0 = 0.0: the tree's own resolution)
            bool tree_wins = true;
            for (size_t j = 0; j < C.size(); ++j) {
                const double d = D[(size_t)C[j] * nrep + r], e = d - mean[j];
                if (e > top) { second = top; top = e; }
                else if (e > second) second = e;
                tree_wins = tree_wins && d <= 0.0;
            }
            if (d_obs > 0.0 && top - second < d_obs) ++s.sh_hits;
            if (tree_wins) ++s.rell_hits;
        }
    }
    ml_support_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
}

}  // namespace pgm
