// treelik_internal.h — what the host statements of the tree likelihood (treelik.cpp, treelik_rates.cpp, treelik_anc.cpp,
// treelik_nni.cpp) share and nobody else needs: the checks, the scaling constants, the pieces of the arithmetic and the walk over
// the tree for one site.
#pragma once
#include "pgm_host.h"
#include "../csrc/pgm_treelik_check.h"

#include <algorithm>
#include <cmath>

namespace pgm {

const double kTreelikTiny = 0x1p-256, kTreelikScale = 0x1p256;
const uint32_t kTreelikChunk = PGM_TREELIK_CHUNK;

// the children of every node in ascending order (CSR), after the checks of the C entry (include/pgm_hip.h: pgm_tree_likelihood;
// csrc/pgm_treelik_check.h holds them for both)
struct TreelikChildren {
    std::vector<uint32_t> tree;   // off (nnodes + 1), then idx (nnodes - 1)
    const uint32_t *off = nullptr, *idx = nullptr;
    TreelikChildren() = default;
    TreelikChildren(TreelikChildren &&) = default;   // (off and idx point into `tree`: moved, never copied)
};
inline TreelikChildren treelik_check_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                          const double *P, int derivs, const double *site_l, const int32_t *site_k, const double *d1, const double *d2) {
    if (!parent || !rows || !pi || !P || !site_l || !site_k || (derivs && (!d1 || !d2))) error("tree likelihood: null argument");
    TreelikChildren ch;
    const std::string bad = pgm_treelik_check_tree(dim, nleaves, nnodes, parent, ncols, rows, ch.tree);
    if (!bad.empty()) error("%s", bad.c_str());
    ch.off = ch.tree.data();
    ch.idx = ch.off + nnodes + 1;
    return ch;
}
// ncat and the weights of the entries with rate categories
inline void treelik_check_rates_host(uint32_t ncat, const double *w) {
    const std::string bad = pgm_treelik_check_rates(ncat, w);
    if (!bad.empty()) error("%s", bad.c_str());
}

// out(i) = sum over j ascending of X(i, j) u(j), u the partial of a child: `u` for an inner node, for a leaf the indicator of its
// value r (r < 0: ones).  A leaf with a state: 0.0 + X(i, r), what the sum gives when every other term is a zero.
inline void treelik_apply(const double *X, uint32_t dim, const double *u, int r, double *out) {
    if (!u && r >= 0) {
        for (uint32_t i = 0; i < dim; ++i) out[i] = 0.0 + X[i + (size_t)dim * (uint32_t)r];
        return;
    }
    for (uint32_t i = 0; i < dim; ++i) out[i] = 0.0;
    for (uint32_t j = 0; j < dim; ++j) {
        const double uj = u ? u[j] : 1.0;
        const double *col = X + (size_t)dim * j;
        for (uint32_t i = 0; i < dim; ++i) out[i] = out[i] + col[i] * uj;
    }
}
// the scaling rule: a vector whose largest entry is below 2^-256 and above 0 is multiplied by 2^256
inline bool treelik_rescale(double *v, uint32_t dim) {
    double m = v[0];
    for (uint32_t i = 1; i < dim; ++i) m = v[i] > m ? v[i] : m;
    if (!(m < kTreelikTiny && m > 0.0)) return false;
    for (uint32_t i = 0; i < dim; ++i) v[i] = v[i] * kTreelikScale;
    return true;
}
// d1[e], d2[e]: the chunk sums of edge e, chunks ascending
inline void treelik_chunk_totals(const std::vector<double> &c1, const std::vector<double> &c2, size_t nchunks, uint32_t nedges, double *d1, double *d2) {
    for (uint32_t e = 0; e < nedges; ++e) {
        double a1 = 0.0, a2 = 0.0;
        for (size_t chunk = 0; chunk < nchunks; ++chunk) { a1 = a1 + c1[chunk * nedges + e]; a2 = a2 + c2[chunk * nedges + e]; }
        d1[e] = a1;
        d2[e] = a2;
    }
}

// The walk over the tree for one site at a time, with the scratch of one thread: the up pass, the scaling rule, and with derivs the
// down pass and the three sums of every edge.  The host statements are loops over it.  posteriors() is the down pass of
// tree_ancestral_host (treelik_anc.cpp): a walk made with derivs == false and anc == true.
struct TreelikSiteWalk {
    const TreelikChildren &ch;
    uint32_t dim, nleaves, nnodes, ncols;
    const int8_t *rows;
    const double *pi;
    bool derivs;
    std::vector<double> U, O, S, base, o, T;
    TreelikSiteWalk(const TreelikChildren &ch_, uint32_t dim_, uint32_t nleaves_, uint32_t nnodes_, uint32_t ncols_, const int8_t *rows_, const double *pi_, bool derivs_,
                    bool anc = false)
        : ch(ch_), dim(dim_), nleaves(nleaves_), nnodes(nnodes_), ncols(ncols_), rows(rows_), pi(pi_), derivs(derivs_) {
        uint32_t max_kids = 2;
        for (uint32_t v = nleaves; v < nnodes; ++v) max_kids = std::max(max_kids, ch.off[v + 1] - ch.off[v]);
        const size_t ninner = nnodes - nleaves;
        U.resize(ninner * dim); O.resize(derivs || anc ? ninner * dim : 0); S.resize((size_t)max_kids * dim); base.resize(dim); o.resize(dim); T.resize(3 * (size_t)dim);
    }
    // site s under the matrices P: (L, k), and with derivs g[e] = A^P' / A^P and q[e] = A^P'' / A^P of every edge e
    void operator()(uint32_t s, const double *P, double &L_out, int32_t &k_out, double *g, double *q) {
        const uint32_t root = nnodes - 1;
        const size_t mat = (size_t)dim * dim, estride = derivs ? 3 * mat : mat;
        auto partial = [&](uint32_t c) -> const double * { return c < nleaves ? nullptr : &U[(size_t)(c - nleaves) * dim]; };
        auto value = [&](uint32_t c) -> int { return c < nleaves ? (int)rows[(size_t)c * ncols + s] : 0; };
        // up pass
        int32_t k = 0;
        for (uint32_t v = nleaves; v < nnodes; ++v) {
            double *Uv = &U[(size_t)(v - nleaves) * dim];
            for (uint32_t qq = ch.off[v]; qq < ch.off[v + 1]; ++qq) {
                const uint32_t c = ch.idx[qq];
                treelik_apply(P + estride * c, dim, partial(c), value(c), S.data());
                if (qq == ch.off[v]) for (uint32_t i = 0; i < dim; ++i) Uv[i] = S[i];
                else for (uint32_t i = 0; i < dim; ++i) Uv[i] = Uv[i] * S[i];
            }
            if (treelik_rescale(Uv, dim)) ++k;
        }
        double L = 0.0;
        for (uint32_t i = 0; i < dim; ++i) L = L + pi[i] * U[(size_t)(root - nleaves) * dim + i];
        L_out = L;
        k_out = k;
        if (!derivs) return;
        // down pass: the outside vector of every edge, then the three sums of the edge
        for (uint32_t v = root; v >= nleaves; --v) {
            if (v == root) for (uint32_t i = 0; i < dim; ++i) base[i] = pi[i];
            else {
                const double *Ov = &O[(size_t)(v - nleaves) * dim], *Pv = P + estride * v;
                for (uint32_t i = 0; i < dim; ++i) {
                    double acc = 0.0;
                    for (uint32_t h = 0; h < dim; ++h) acc = acc + Ov[h] * Pv[h + (size_t)dim * i];
                    base[i] = acc;
                }
            }
            const uint32_t q0 = ch.off[v], q1 = ch.off[v + 1];
            for (uint32_t qq = q0; qq < q1; ++qq) treelik_apply(P + estride * ch.idx[qq], dim, partial(ch.idx[qq]), value(ch.idx[qq]), &S[(size_t)(qq - q0) * dim]);
            for (uint32_t qq = q0; qq < q1; ++qq) {
                const uint32_t c = ch.idx[qq];
                for (uint32_t i = 0; i < dim; ++i) o[i] = base[i];
                for (uint32_t r = q0; r < q1; ++r)
                    if (r != qq) for (uint32_t i = 0; i < dim; ++i) o[i] = o[i] * S[(size_t)(r - q0) * dim + i];
                treelik_rescale(o.data(), dim);
                if (c >= nleaves) std::copy(o.begin(), o.end(), O.begin() + (size_t)(c - nleaves) * dim);
                double A[3];
                for (int x = 0; x < 3; ++x) {
                    if (x == 0) std::copy(S.begin() + (size_t)(qq - q0) * dim, S.begin() + (size_t)(qq - q0 + 1) * dim, T.begin());
                    else treelik_apply(P + estride * c + mat * x, dim, partial(c), value(c), T.data());
                    double acc = 0.0;
                    for (uint32_t i = 0; i < dim; ++i) acc = acc + o[i] * T[i];
                    A[x] = acc;
                }
                g[c] = A[1] / A[0];
                q[c] = A[2] / A[0];
            }
        }
    }
    // After operator() on site s under the same P (P alone: derivs == false): the down pass with S from P, and per inner node v
    // a[(v - nleaves) * dim + i] = m(i) / Z with m(i) = B_v(i) U_v(i), Z = sum_i m(i) ascending; 0.0 where Z == 0.0
    void posteriors(uint32_t s, const double *P, double *a) {
        const uint32_t root = nnodes - 1;
        const size_t mat = (size_t)dim * dim;
        auto partial = [&](uint32_t c) -> const double * { return c < nleaves ? nullptr : &U[(size_t)(c - nleaves) * dim]; };
        auto value = [&](uint32_t c) -> int { return c < nleaves ? (int)rows[(size_t)c * ncols + s] : 0; };
        for (uint32_t v = root; v >= nleaves; --v) {
            if (v == root) for (uint32_t i = 0; i < dim; ++i) base[i] = pi[i];
            else {
                const double *Ov = &O[(size_t)(v - nleaves) * dim], *Pv = P + mat * v;
                for (uint32_t i = 0; i < dim; ++i) {
                    double acc = 0.0;
                    for (uint32_t h = 0; h < dim; ++h) acc = acc + Ov[h] * Pv[h + (size_t)dim * i];
                    base[i] = acc;
                }
            }
            if (a) {   // (null: the outside vectors alone, what tree_nni_host reads)
                const double *Uv = &U[(size_t)(v - nleaves) * dim];
                double *av = a + (size_t)(v - nleaves) * dim, Z = 0.0;
                for (uint32_t i = 0; i < dim; ++i) { av[i] = base[i] * Uv[i]; Z = Z + av[i]; }
                for (uint32_t i = 0; i < dim; ++i) av[i] = Z == 0.0 ? 0.0 : av[i] / Z;
            }
            const uint32_t q0 = ch.off[v], q1 = ch.off[v + 1];
            for (uint32_t qq = q0; qq < q1; ++qq) treelik_apply(P + mat * ch.idx[qq], dim, partial(ch.idx[qq]), value(ch.idx[qq]), &S[(size_t)(qq - q0) * dim]);
            for (uint32_t qq = q0; qq < q1; ++qq) {
                const uint32_t c = ch.idx[qq];
                if (c < nleaves) continue;   // (a leaf's outside vector has no reader)
                double *Oc = &O[(size_t)(c - nleaves) * dim];
                for (uint32_t i = 0; i < dim; ++i) Oc[i] = base[i];
                for (uint32_t r = q0; r < q1; ++r)
                    if (r != qq) for (uint32_t i = 0; i < dim; ++i) Oc[i] = Oc[i] * S[(size_t)(r - q0) * dim + i];
                treelik_rescale(Oc, dim);
            }
        }
    }
};

}  // namespace pgm
