// treelik_joint.cpp — joint ancestral reconstruction and samples from the posterior for `pgmsa --ml_tree --ml_ancestral_joint` and
// `--ml_ancestral_samples` (the walk and the checks are treelik_internal.h's): the host statements of
// pgm_tree_ancestral_joint and pgm_tree_ancestral_sample (Backend::tree_ancestral_joint's and Backend::tree_ancestral_sample's
// defaults, what pgmsa_oracle runs).
#include "treelik_internal.h"

namespace pgm {

namespace {
// The up pass of every category at site s (the partials of category c into U + c * ustride) and the combine of
// tree_likelihood_rates_host: site_l, site_k and post of the site; term: ncat doubles of scratch, the posteriors on return.
void joint_site_values(TreelikSiteWalk &walk, uint32_t s, uint32_t ncols, uint32_t ncat, const double *w, const double *P, size_t pstride, double *U, size_t ustride,
                       std::vector<double> &L, std::vector<int32_t> &k, std::vector<double> &term, double *site_l, int32_t *site_k, double *post) {
    for (uint32_t c = 0; c < ncat; ++c) {
        walk(s, P + pstride * c, L[c], k[c], nullptr, nullptr);
        if (U) std::copy(walk.U.begin(), walk.U.end(), U + ustride * c);
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
}

// u of the draw numbered `counter` (include/pgm_hip.h: pgm_tree_ancestral_sample): splitmix64's own first addition gives counter + 1
double sample_uniform(uint64_t seed, uint64_t counter) {
    uint64_t state = seed + 0x9E3779B97F4A7C15ull * counter;
    return (double)(splitmix64(state) >> 11) * 0x1p-53;
}
// the pick rule of the interface on the weights weight(0) .. weight(m - 1)
template <class W> int sample_pick(uint32_t m, double u, W weight) {
    double T = 0.0;
    for (uint32_t j = 0; j < m; ++j) T = T + weight(j);
    if (T == 0.0) return -1;
    const double target = u * T;
    double c = 0.0;
    int last = -1;
    for (uint32_t j = 0; j < m; ++j) {
        const double q = weight(j);
        c = c + q;
        if (c > target) return (int)j;
        if (q > 0.0) last = (int)j;
    }
    return last;
}
}  // namespace

void tree_ancestral_joint_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                               const double *w, const double *P, double *site_l, int32_t *site_k, double *post, uint8_t *cat, int8_t *joint_state, double *joint_l,
                               int32_t *joint_k) {
    if (!w || !post || !cat || !joint_state || !joint_l || !joint_k) error("tree likelihood: null argument");
    treelik_check_rates_host(ncat, w);
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, 0, site_l, site_k, nullptr, nullptr);
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves, root = nnodes - 1;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk, mat = (size_t)dim * dim, pstride = mat * nedges;

    parallel_for(nchunks, [&](size_t chunk) {
        TreelikSiteWalk walk(ch, dim, nleaves, nnodes, ncols, rows, pi, false);
        std::vector<double> L(ncat), term(ncat), F((size_t)ninner * dim), m(dim);
        std::vector<int32_t> k(ncat);
        std::vector<uint8_t> ptr((size_t)ninner * dim);
        const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
        for (uint32_t s = s0; s < s1; ++s) {
            joint_site_values(walk, s, ncols, ncat, w, P, pstride, nullptr, 0, L, k, term, site_l, site_k, post);
            uint32_t best_cat = 0;
            for (uint32_t c = 1; c < ncat; ++c) if (term[c] > term[best_cat]) best_cat = c;
            const double *Pk = P + pstride * best_cat;
            // the max pass: F of every inner node ascending, the back-pointers of every inner node below the root
            int32_t count = 0;
            for (uint32_t v = nleaves; v < nnodes; ++v) {
                double *Fv = &F[(size_t)(v - nleaves) * dim];
                for (uint32_t q = ch.off[v]; q < ch.off[v + 1]; ++q) {
                    const uint32_t c = ch.idx[q];
                    if (c < nleaves) treelik_apply(Pk + mat * c, dim, nullptr, (int)rows[(size_t)c * ncols + s], m.data());
                    else {
                        const double *X = Pk + mat * c, *Fc = &F[(size_t)(c - nleaves) * dim];
                        for (uint32_t i = 0; i < dim; ++i) {
                            double top = X[i] * Fc[0];
                            uint32_t arg = 0;
                            for (uint32_t j = 1; j < dim; ++j) { const double x = X[i + (size_t)dim * j] * Fc[j]; if (x > top) { top = x; arg = j; } }
                            m[i] = top;
                            ptr[(size_t)(c - nleaves) * dim + i] = (uint8_t)arg;
                        }
                    }
                    if (q == ch.off[v]) for (uint32_t i = 0; i < dim; ++i) Fv[i] = m[i];
                    else for (uint32_t i = 0; i < dim; ++i) Fv[i] = Fv[i] * m[i];
                }
                if (treelik_rescale(Fv, dim)) ++count;
            }
            const double *Fr = &F[(size_t)(root - nleaves) * dim];
            double top = pi[0] * Fr[0];
            uint32_t arg = 0;
            for (uint32_t j = 1; j < dim; ++j) { const double x = pi[j] * Fr[j]; if (x > top) { top = x; arg = j; } }
            joint_l[s] = top;
            joint_k[s] = count;
            cat[s] = (uint8_t)best_cat;
            joint_state[(size_t)(root - nleaves) * ncols + s] = top == 0.0 ? (int8_t)-1 : (int8_t)arg;
            for (uint32_t v = root; v-- > nleaves;) {   // parents first
                const int up = joint_state[(size_t)(parent[v] - nleaves) * ncols + s];
                joint_state[(size_t)(v - nleaves) * ncols + s] = up < 0 ? (int8_t)-1 : (int8_t)ptr[(size_t)(v - nleaves) * dim + (uint32_t)up];
            }
        }
    });
}

void tree_ancestral_sample_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                                const double *w, const double *P, uint32_t nsamp, uint64_t first_sample, uint64_t seed, double *site_l, int32_t *site_k, double *post,
                                uint8_t *samp_cat, int8_t *samp_state) {
    if (!w || !post || !samp_cat || !samp_state) error("tree likelihood: null argument");
    if (nsamp == 0) error("tree ancestral sample: no sample");
    treelik_check_rates_host(ncat, w);
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, 0, site_l, site_k, nullptr, nullptr);
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves, root = nnodes - 1;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk, mat = (size_t)dim * dim, pstride = mat * nedges, ustride = (size_t)ninner * dim;

    parallel_for(nchunks, [&](size_t chunk) {
        TreelikSiteWalk walk(ch, dim, nleaves, nnodes, ncols, rows, pi, false);
        std::vector<double> L(ncat), term(ncat), U((size_t)ncat * ustride);
        std::vector<int32_t> k(ncat);
        const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
        for (uint32_t s = s0; s < s1; ++s) {
            joint_site_values(walk, s, ncols, ncat, w, P, pstride, U.data(), ustride, L, k, term, site_l, site_k, post);
            for (uint32_t n = 0; n < nsamp; ++n) {
                const uint64_t N = first_sample + n, base = (N * ncols + s) * ((uint64_t)ninner + 1);
                auto state_of = [&](uint32_t v) -> int8_t & { return samp_state[((size_t)(v - nleaves) * ncols + s) * nsamp + n]; };
                const int kk = sample_pick(ncat, sample_uniform(seed, base), [&](uint32_t c) { return term[c]; });
                samp_cat[(size_t)s * nsamp + n] = (uint8_t)kk;   // (-1: 255)
                const double *Pk = P + pstride * (size_t)(kk < 0 ? 0 : kk), *Uk = U.data() + ustride * (size_t)(kk < 0 ? 0 : kk);
                int x = -1;
                if (kk >= 0) {
                    const double *u = Uk + (size_t)(root - nleaves) * dim;
                    x = sample_pick(dim, sample_uniform(seed, base + 1 + (root - nleaves)), [&](uint32_t j) { return pi[j] * u[j]; });
                }
                state_of(root) = (int8_t)x;
                for (uint32_t v = root; v-- > nleaves;) {   // parents first
                    const int up = state_of(parent[v]);
                    x = -1;
                    if (up >= 0) {
                        const double *row = Pk + mat * v + (uint32_t)up, *u = Uk + (size_t)(v - nleaves) * dim;
                        x = sample_pick(dim, sample_uniform(seed, base + 1 + (v - nleaves)), [&](uint32_t j) { return row[(size_t)dim * j] * u[j]; });
                    }
                    state_of(v) = (int8_t)x;
                }
            }
        }
    });
}

void Backend::tree_ancestral_joint(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                                   const double *w, const double *P, double *site_l, int32_t *site_k, double *post, uint8_t *cat, int8_t *joint_state, double *joint_l,
                                   int32_t *joint_k, int) {
    tree_ancestral_joint_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, site_l, site_k, post, cat, joint_state, joint_l, joint_k);
}
void Backend::tree_ancestral_sample(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                                    const double *w, const double *P, uint32_t nsamp, uint64_t first_sample, uint64_t seed, double *site_l, int32_t *site_k, double *post,
                                    uint8_t *samp_cat, int8_t *samp_state, int) {
    tree_ancestral_sample_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, nsamp, first_sample, seed, site_l, site_k, post, samp_cat, samp_state);
}

}  // namespace pgm
