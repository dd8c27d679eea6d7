// treelik_anc.cpp — marginal ancestral states for `pgmsa --ml_tree --ml_ancestral` (the walk and the checks are
// treelik_internal.h's): the host statement of pgm_tree_ancestral
// (Backend::tree_ancestral's default, what pgmsa_oracle runs).
#include "treelik_internal.h"

namespace pgm {

void tree_ancestral_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                         const double *w, const double *P, double *site_l, int32_t *site_k, double *post, int8_t *anc_state, double *anc_prob, double *anc_post) {
    if (!w || !post || !anc_state || !anc_prob) error("tree likelihood: null argument");
    treelik_check_rates_host(ncat, w);
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, 0, site_l, site_k, nullptr, nullptr);
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk, pstride = (size_t)dim * dim * nedges, astride = (size_t)ninner * dim;

    parallel_for(nchunks, [&](size_t chunk) {
        TreelikSiteWalk walk(ch, dim, nleaves, nnodes, ncols, rows, pi, false, true);
        std::vector<double> a((size_t)ncat * astride), L(ncat), term(ncat), anc(dim);
        std::vector<int32_t> k(ncat);
        const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
        for (uint32_t s = s0; s < s1; ++s) {
            for (uint32_t c = 0; c < ncat; ++c) {
                walk(s, P + pstride * c, L[c], k[c], nullptr, nullptr);
                walk.posteriors(s, P + pstride * c, &a[(size_t)c * astride]);
            }
            int32_t kmin = k[0];
            for (uint32_t c = 1; c < ncat; ++c) kmin = k[c] < kmin ? k[c] : kmin;
            double total = 0.0;
            for (uint32_t c = 0; c < ncat; ++c) {
                double t = w[c] * L[c];
                for (int32_t d = k[c] - kmin; d > 0; --d) t = t * kTreelikTiny;
                term[c] = t;
                total = total + t;
            }
            site_l[s] = total;
            site_k[s] = kmin;
            for (uint32_t c = 0; c < ncat; ++c) { term[c] = term[c] / total; post[(size_t)c * ncols + s] = term[c]; }
            for (uint32_t row = 0; row < ninner; ++row) {
                int best = -1;
                double top = 0.0;
                for (uint32_t i = 0; i < dim; ++i) {
                    double x = 0.0;
                    for (uint32_t c = 0; c < ncat; ++c) x = x + term[c] * a[(size_t)c * astride + (size_t)row * dim + i];
                    if (anc_post) anc_post[((size_t)row * ncols + s) * dim + i] = x;
                    if (x > top) { top = x; best = (int)i; }
                }
                anc_state[(size_t)row * ncols + s] = (int8_t)best;
                anc_prob[(size_t)row * ncols + s] = top;
            }
        }
    });
}

// The gap rule of --ml_ancestral: r(x) = the leaves below x whose row is not -1; a node is present at a column iff at least two of
// the directions at it (its children, and its parent's side unless it is the root) hold such a leaf.  Integer work.
void tree_ancestral_presence(uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, uint8_t *present) {
    if (!parent || !rows || !present || nleaves < 2 || nnodes <= nleaves || ncols == 0) error("tree ancestral presence: bad argument");
    const uint32_t root = nnodes - 1, ninner = nnodes - nleaves;
    for (uint32_t v = 0; v < root; ++v)
        if (parent[v] <= v || parent[v] < nleaves || parent[v] >= nnodes) error("tree ancestral presence: the parent of node %u is not an inner node above it", v);
    std::vector<uint32_t> below((size_t)nnodes * ncols, 0), sides((size_t)ninner * ncols, 0);
    for (uint32_t v = 0; v < root; ++v) {   // (children before parents: r(v) is complete when v is reached)
        uint32_t *rv = &below[(size_t)v * ncols], *rp = &below[(size_t)parent[v] * ncols], *sp = &sides[(size_t)(parent[v] - nleaves) * ncols];
        for (uint32_t s = 0; s < ncols; ++s) {
            if (v < nleaves) rv[s] = rows[(size_t)v * ncols + s] != -1 ? 1u : 0u;
            rp[s] += rv[s];
            sp[s] += rv[s] > 0 ? 1u : 0u;
        }
    }
    for (uint32_t v = nleaves; v < nnodes; ++v)
        for (uint32_t s = 0; s < ncols; ++s) {
            const uint32_t up = v != root && below[(size_t)root * ncols + s] - below[(size_t)v * ncols + s] > 0 ? 1u : 0u;
            present[(size_t)(v - nleaves) * ncols + s] = sides[(size_t)(v - nleaves) * ncols + s] + up >= 2 ? 1 : 0;
        }
}

void Backend::tree_ancestral(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                             const double *w, const double *P, double *site_l, int32_t *site_k, double *post, int8_t *anc_state, double *anc_prob, double *anc_post, int) {
    tree_ancestral_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, site_l, site_k, post, anc_state, anc_prob, anc_post);
}

}  // namespace pgm
