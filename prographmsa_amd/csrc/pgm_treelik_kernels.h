// pgm_treelik_kernels.h — Felsenstein pruning for pgm_tree_likelihood (include/pgm_hip.h), plain form.
//
// Columns are independent: a workgroup of one wavefront owns 64 / dim consecutive sites and walks the whole tree itself, one thread
// per (site, state).  The up pass goes over the inner nodes in ascending order (children come before parents), the down pass and
// the per-edge ratios over them in descending order; the partials and the outside vectors of the inner nodes live in global memory,
// written and read by the same workgroup only (__syncthreads between a node and its parent).  No workgroup waits for another,
// nothing spins, there are no atomics.  The matrices of the edge in hand are read from global memory by every thread (lanes of one
// site read consecutive entries of a column; the 3.2 KB to 98 KB of an edge stay in the vector L1 / L2 while the workgroups pass it).
// pgm_treelik_sums_kernel adds the per-site ratios of an edge in the fixed order of the interface.
// pgm_tree_likelihood_rates runs the same walk once per rate category, the categories as further workgroups of one
// launch (pgm_treelik_cat_kernel), and combines them per site (pgm_treelik_combine_kernel) ahead of the sums.
// pgm_tree_ancestral is a third mode of the walk (PGM_TREELIK_ANC): the down pass with P alone, the posterior
// of every inner node's states written where the node's outside vector was; pgm_treelik_anc_combine_kernel mixes the categories.
// pgm_tree_nni is a fourth mode (PGM_TREELIK_NNI): that down pass without the posteriors, so the outside
// vectors stay; pgm_treelik_nni_kernel then scores every nearest-neighbour interchange from four stored pieces around its edge.
// pgm_tree_nni_edge is that kernel's second instantiation: the neighbour's edge with three matrices of its own.
// pgm_tree_spr runs the walk in the same mode; pgm_treelik_spr_kernel then scores every pruning and regrafting from
// the stored pieces along the candidate's path.
// pgm_tree_ancestral_joint and pgm_tree_ancestral_sample run the walk as pgm_tree_likelihood_rates does without
// derivs and then kernels of their own, at the end of this file: a max-product pass with back-pointers and its traceback, and a
// stochastic traceback through the stored partials.
//
// Every sum over states runs ascending from 0.0 with one multiply and one add per term (-ffp-contract=off): the bits are those of
// tree_likelihood_host.  The walk is a chain of dependent steps on one wavefront, so what a step costs is the latency of its loads:
// the sums fetch eight terms' operands ahead of the eight adds (the adds keep their order), the three sums of an edge (P, P', P'')
// share one pass over the child's partial, and a leaf with a state reads its one column.
#ifndef PGM_TREELIK_KERNELS_H_
#define PGM_TREELIK_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGM_TREELIK_THREADS 64

struct PgmTreelikArgs {
    uint32_t dim, nleaves, nnodes, ncols, spb;   // spb: sites per workgroup = 64 / dim
    int derivs;
    const uint32_t *child_off, *child;           // CSR: the children of every node, ascending
    const int8_t *rows;
    const double *pi, *P;
    double *U, *O;                               // (nnodes - nleaves) x ncols x dim each; O only with derivs (and in the ancestral mode)
    double *g, *h;                               // (nnodes - 1) x ncols each, derivs only
    double *site_l;
    int32_t *site_k;
};

// acc[x] = sum over j ascending of X_x(i, j) u_c(j) for this thread's state i and site s, X_x the NX matrices of edge c back to back
// (`mat` doubles apart): u_c the stored partial of an inner node, the indicator of the row value for a leaf.  A leaf with a state r:
// 0.0 + X_x(i, r), what the sum gives when every other term is a zero; a leaf without one: the terms are the entries themselves.
template <int NX>
__device__ __forceinline__ void pgm_treelik_apply(const PgmTreelikArgs &a, const double *X, size_t mat, uint32_t c, uint32_t s, uint32_t i, double (&acc)[NX]) {
    const uint32_t dim = a.dim;
    const double *col = X + i;
#pragma unroll
    for (int x = 0; x < NX; ++x) acc[x] = 0.0;
    if (c < a.nleaves) {
        const int r = a.rows[(size_t)c * a.ncols + s];
        if (r >= 0) {
#pragma unroll
            for (int x = 0; x < NX; ++x) acc[x] = 0.0 + col[mat * x + (size_t)dim * (uint32_t)r];
            return;
        }
        uint32_t j = 0;
        for (; j + 8 <= dim; j += 8) {
            double xv[NX][8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
#pragma unroll
                for (int x = 0; x < NX; ++x) xv[x][q] = col[mat * x + (size_t)dim * (j + q)];
#pragma unroll
            for (int q = 0; q < 8; ++q)
#pragma unroll
                for (int x = 0; x < NX; ++x) acc[x] = acc[x] + xv[x][q];
        }
        for (; j < dim; ++j)
#pragma unroll
            for (int x = 0; x < NX; ++x) acc[x] = acc[x] + col[mat * x + (size_t)dim * j];
        return;
    }
    const double *u = a.U + ((size_t)(c - a.nleaves) * a.ncols + s) * dim;
    uint32_t j = 0;
    for (; j + 8 <= dim; j += 8) {
        double xv[NX][8], uv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            uv[q] = u[j + q];
#pragma unroll
            for (int x = 0; x < NX; ++x) xv[x][q] = col[mat * x + (size_t)dim * (j + q)];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int x = 0; x < NX; ++x) acc[x] = acc[x] + xv[x][q] * uv[q];
    }
    for (; j < dim; ++j) {
        const double uj = u[j];
#pragma unroll
        for (int x = 0; x < NX; ++x) acc[x] = acc[x] + col[mat * x + (size_t)dim * j] * uj;
    }
}

// the scaling rule on the dim values of a site, one per thread: true when the values were multiplied by 2^256.
// sh: this site's dim doubles of shared memory.  Every thread of the workgroup calls it (two barriers).
__device__ __forceinline__ bool pgm_treelik_rescale(double &v, double *sh, uint32_t dim, uint32_t i, bool active) {
    __syncthreads();
    if (active) sh[i] = v;
    __syncthreads();
    bool scaled = false;
    if (active) {
        double m = sh[0];
#pragma unroll 8
        for (uint32_t k = 1; k < dim; ++k) m = sh[k] > m ? sh[k] : m;
        scaled = m < 0x1p-256 && m > 0.0;
        if (scaled) v = v * 0x1p256;
    }
    return scaled;
}

// One edge of the down pass, for the dim threads of a site: the outside vector o (before its scaling) and T[x] = sum_j X_x(i, j) U_c(j)
// of this thread's state.  Scales o, stores it for an inner child, and the thread of state 0 adds the three sums over the states
// ascending and writes the two ratios: g and h = A''/A - g g, or with RAW (a category of pgm_tree_likelihood_rates) g and q = A''/A.
// Every thread of the workgroup calls it (barriers).
template <bool RAW>
__device__ __forceinline__ void pgm_treelik_edge(const PgmTreelikArgs &a, double (*sh)[PGM_TREELIK_THREADS], double *shs, uint32_t c, uint32_t s, uint32_t i,
                                                 bool active, double o, const double (&T)[3]) {
    const uint32_t dim = a.dim;
    (void)pgm_treelik_rescale(o, shs, dim, i, active);
    if (active && c >= a.nleaves) a.O[((size_t)(c - a.nleaves) * a.ncols + s) * dim + i] = o;
    __syncthreads();   // (the maximum's reads of sh[0] are done)
    if (active) {
        sh[0][threadIdx.x] = o * T[0];
        sh[1][threadIdx.x] = o * T[1];
        sh[2][threadIdx.x] = o * T[2];
    }
    __syncthreads();
    if (active && i == 0) {
        double A0 = 0.0, A1 = 0.0, A2 = 0.0;
#pragma unroll 8
        for (uint32_t j = 0; j < dim; ++j) {
            A0 = A0 + sh[0][threadIdx.x + j];
            A1 = A1 + sh[1][threadIdx.x + j];
            A2 = A2 + sh[2][threadIdx.x + j];
        }
        const double g = A1 / A0;
        a.g[(size_t)c * a.ncols + s] = g;
        a.h[(size_t)c * a.ncols + s] = RAW ? A2 / A0 : A2 / A0 - g * g;
    }
}

// The ancestral mode's step at node v, for the dim threads of a site: m(i) = B_v(i) U_v(i), Z = sum of m ascending, and m / Z (0.0
// where Z == 0.0) into the slot of O_v, which is dead once `base` = B_v(i) is formed (the root's slot has no other use).  The barrier
// stands between the last read of O_v by the site's threads and the overwrite, and publishes m; every thread of a site then adds the
// same dim values in the same order (one LDS address per site: a broadcast), which spares the barrier a broadcast of Z would need.
// Every thread of the workgroup calls it.
__device__ __forceinline__ void pgm_treelik_posterior(const PgmTreelikArgs &a, double *sh0, uint32_t v, uint32_t s, uint32_t i, bool active, double base) {
    const uint32_t dim = a.dim;
    const size_t at = ((size_t)(v - a.nleaves) * a.ncols + s) * dim + i;
    double m = 0.0;
    if (active) { m = base * a.U[at]; sh0[threadIdx.x] = m; }
    __syncthreads();
    if (active) {
        const double *ms = sh0 + (threadIdx.x - i);
        double Z = 0.0;
#pragma unroll 8
        for (uint32_t j = 0; j < dim; ++j) Z = Z + ms[j];
        a.O[at] = Z == 0.0 ? 0.0 : m / Z;
    }
}

// The walk of one workgroup over the whole tree for the sites of block blockIdx.x: the kernels below are this function.  MODE:
// PGM_TREELIK_PLAIN (pgm_tree_likelihood), PGM_TREELIK_RAW (a category of pgm_tree_likelihood_rates: q in place of h),
// PGM_TREELIK_ANC (a category of pgm_tree_ancestral: P alone, posteriors in place of the edges' sums), PGM_TREELIK_NNI (a category of
// pgm_tree_nni: the ANC mode without the posteriors, the outside vector of every inner node but the root stays in a.O).
enum { PGM_TREELIK_PLAIN = 0, PGM_TREELIK_RAW = 1, PGM_TREELIK_ANC = 2, PGM_TREELIK_NNI = 3 };
template <int MODE>
__device__ __forceinline__ void pgm_treelik_walk(const PgmTreelikArgs &a) {
    constexpr bool RAW = MODE == PGM_TREELIK_RAW, PALONE = MODE == PGM_TREELIK_ANC || MODE == PGM_TREELIK_NNI;
    __shared__ double sh[3][PGM_TREELIK_THREADS];
    const uint32_t dim = a.dim, nleaves = a.nleaves, root = a.nnodes - 1;
    const uint32_t local = threadIdx.x / dim, i = threadIdx.x - local * dim;
    const uint64_t s64 = (uint64_t)blockIdx.x * a.spb + local;
    const bool active = local < a.spb && s64 < a.ncols;
    const uint32_t s = (uint32_t)s64;
    const size_t mat = (size_t)dim * dim, estride = a.derivs ? 3 * mat : mat;
    double *shs = &sh[0][local * dim];   // (local * dim + i == threadIdx.x < 64)

    // up pass
    int32_t k = 0;
    for (uint32_t v = nleaves; v <= root; ++v) {
        double prod = 0.0;
        if (active) {
            const uint32_t q0 = a.child_off[v], q1 = a.child_off[v + 1];
            for (uint32_t q = q0; q < q1; ++q) {
                const uint32_t c = a.child[q];
                double S[1];
                pgm_treelik_apply<1>(a, a.P + estride * c, mat, c, s, i, S);
                prod = q == q0 ? S[0] : prod * S[0];
            }
        }
        if (pgm_treelik_rescale(prod, shs, dim, i, active)) ++k;
        if (active) a.U[((size_t)(v - nleaves) * a.ncols + s) * dim + i] = prod;
        __syncthreads();   // the node's partial is in memory before its parent reads it
    }
    {   // the site likelihood: sum over the states ascending
        const double *u = a.U + ((size_t)(root - nleaves) * a.ncols + s) * dim;
        if (active && i == 0) {
            double L = 0.0;
#pragma unroll 8
            for (uint32_t j = 0; j < dim; ++j) L = L + a.pi[j] * u[j];
            a.site_l[s] = L;
            a.site_k[s] = k;
        }
    }
    if (!PALONE && !a.derivs) return;

    // down pass, parents before children: the outside vector of every edge below v, then the edge's three sums
    for (uint32_t v = root; v >= nleaves; --v) {
        double base = 0.0;
        const uint32_t q0 = a.child_off[v], q1 = a.child_off[v + 1];   // (uniform over the workgroup: the barriers below)
        if (active) {
            if (v == root) base = a.pi[i];
            else {
                const double *o = a.O + ((size_t)(v - nleaves) * a.ncols + s) * dim, *Pv = a.P + estride * v + (size_t)dim * i;
                uint32_t h = 0;
                for (; h + 8 <= dim; h += 8) {
                    double ov[8], pv[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) { ov[q] = o[h + q]; pv[q] = Pv[h + q]; }
#pragma unroll
                    for (int q = 0; q < 8; ++q) base = base + ov[q] * pv[q];
                }
                for (; h < dim; ++h) base = base + o[h] * Pv[h];
            }
        }
        if (PALONE) {
            // the node's posterior, then the outside vectors of its inner children only: a leaf's has no reader
            if (MODE == PGM_TREELIK_ANC) pgm_treelik_posterior(a, &sh[0][0], v, s, i, active, base);
            for (uint32_t q = q0; q < q1; ++q) {
                const uint32_t c = a.child[q];
                if (c < nleaves) continue;   // (uniform over the workgroup)
                double o = base;
                if (active) {
                    for (uint32_t r = q0; r < q1; ++r) {
                        if (r == q) continue;
                        const uint32_t sib = a.child[r];
                        double S[1];
                        pgm_treelik_apply<1>(a, a.P + estride * sib, mat, sib, s, i, S);
                        o = o * S[0];
                    }
                }
                (void)pgm_treelik_rescale(o, shs, dim, i, active);   // (its first barrier: the posterior's reads of sh are done)
                if (active) a.O[((size_t)(c - nleaves) * a.ncols + s) * dim + i] = o;
            }
        } else if (q1 - q0 == 2) {   // two children: the sibling's S is the other child's own first sum
            const uint32_t c0 = a.child[q0], c1 = a.child[q0 + 1];
            double T0[3] = {0.0, 0.0, 0.0}, T1[3] = {0.0, 0.0, 0.0};
            if (active) {
                pgm_treelik_apply<3>(a, a.P + estride * c0, mat, c0, s, i, T0);
                pgm_treelik_apply<3>(a, a.P + estride * c1, mat, c1, s, i, T1);
            }
            pgm_treelik_edge<RAW>(a, sh, shs, c0, s, i, active, base * T1[0], T0);
            pgm_treelik_edge<RAW>(a, sh, shs, c1, s, i, active, base * T0[0], T1);
        } else {
            for (uint32_t q = q0; q < q1; ++q) {
                const uint32_t c = a.child[q];
                double o = base, T[3] = {0.0, 0.0, 0.0};
                if (active) {
                    for (uint32_t r = q0; r < q1; ++r) {
                        const uint32_t sib = a.child[r];
                        if (r == q) pgm_treelik_apply<3>(a, a.P + estride * sib, mat, sib, s, i, T);
                        else {
                            double S[1];
                            pgm_treelik_apply<1>(a, a.P + estride * sib, mat, sib, s, i, S);
                            o = o * S[0];
                        }
                    }
                }
                pgm_treelik_edge<RAW>(a, sh, shs, c, s, i, active, o, T);
            }
        }
        __syncthreads();   // the children's outside vectors are in memory before they are parents themselves
    }
}

__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_kernel(PgmTreelikArgs a) { pgm_treelik_walk<PGM_TREELIK_PLAIN>(a); }

// The walk once per rate category: category blockIdx.y walks the tree with its own matrices, partials and
// outputs, `a` holding those of category 0 and the strides the distance between two categories.  The categories are independent
// workgroups of one launch.  a.site_l / a.site_k get (L_c, k_c).  MODE PGM_TREELIK_RAW (pgm_tree_likelihood_rates): with derivs
// a.g / a.h get the ratios (g_c, q_c) of every edge and site.  PGM_TREELIK_ANC (pgm_tree_ancestral; P alone: a.derivs == 0): the
// posteriors a_c,v land in a.O, [v - nleaves][s][i], the layout of the outside vectors they replace.  PGM_TREELIK_NNI (pgm_tree_nni):
// as ANC, but a.O keeps the outside vectors O_v.
struct PgmTreelikRatesStride { size_t P, U, G, L; };   // doubles between the categories' matrices, partials, ratios, site values
template <int MODE>
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_cat_kernel(PgmTreelikArgs a, PgmTreelikRatesStride st) {
    const size_t c = blockIdx.y;
    a.P += st.P * c;
    a.U += st.U * c;
    a.site_l += st.L * c;
    a.site_k += st.L * c;
    if constexpr (MODE == PGM_TREELIK_RAW) {
        if (a.derivs) { a.O += st.U * c; a.g += st.G * c; a.h += st.G * c; }
    } else a.O += st.U * c;
    pgm_treelik_walk<MODE>(a);
}

// The categories of a site combined in the order of the interface.  A workgroup owns 64 consecutive sites (reads and writes run along
// the sites); its thread computes site_k = min_c k_c, term_c = w_c L_c times 2^-256 (k_c - site_k) times, site_l = sum_c term_c and
// post_c = term_c / site_l, and keeps post in shared memory.  The workgroups of blockIdx.y == 0 write these; then every workgroup
// takes the edges blockIdx.y, blockIdx.y + gridDim.y, ... and writes g = sum_c post_c g_c and h = sum_c post_c q_c - g g of its
// sites.  Every entry has one writer.
struct PgmTreelikCombineArgs {
    uint32_t ncat, ncols, nedges;
    const double *w, *L;         // ncat; ncat x ncols
    const int32_t *k;            // ncat x ncols
    const double *gc, *qc;       // ncat x nedges x ncols each (nedges == 0: none)
    double *site_l, *post, *g, *h;
    int32_t *site_k;
};
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_combine_kernel(PgmTreelikCombineArgs a) {
    __shared__ double post[PGM_TREELIK_MAXCAT][PGM_TREELIK_THREADS];
    const uint64_t s64 = (uint64_t)blockIdx.x * PGM_TREELIK_THREADS + threadIdx.x;
    if (s64 >= a.ncols) return;   // (no barrier below: a thread reads its own column of `post` only)
    const size_t s = (size_t)s64, ncols = a.ncols;
    int32_t kmin = a.k[s];
    for (uint32_t c = 1; c < a.ncat; ++c) { const int32_t kc = a.k[c * ncols + s]; kmin = kc < kmin ? kc : kmin; }
    double total = 0.0;
    for (uint32_t c = 0; c < a.ncat; ++c) {
        double term = a.w[c] * a.L[c * ncols + s];
        for (int32_t d = a.k[c * ncols + s] - kmin; d > 0; --d) term = term * 0x1p-256;
        post[c][threadIdx.x] = term;
        total = total + term;
    }
    for (uint32_t c = 0; c < a.ncat; ++c) post[c][threadIdx.x] = post[c][threadIdx.x] / total;
    if (blockIdx.y == 0) {
        a.site_l[s] = total;
        a.site_k[s] = kmin;
        for (uint32_t c = 0; c < a.ncat; ++c) a.post[c * ncols + s] = post[c][threadIdx.x];
    }
    const size_t cat = (size_t)a.nedges * ncols;
    for (uint32_t e = blockIdx.y; e < a.nedges; e += gridDim.y) {
        const size_t at = (size_t)e * ncols + s;
        double g = 0.0, q = 0.0;
        for (uint32_t c = 0; c < a.ncat; ++c) {
            g = g + post[c][threadIdx.x] * a.gc[cat * c + at];
            q = q + post[c][threadIdx.x] * a.qc[cat * c + at];
        }
        a.g[at] = g;
        a.h[at] = q - g * g;
    }
}

// The categories' posteriors of pgm_tree_ancestral mixed, and the first state of the largest.  The (node, site) pairs are numbered
// g = (v - nleaves) * ncols + s, so a_c is one array of npairs x dim doubles per category and consecutive lanes read consecutive
// doubles; a wavefront holds 64 / dim pairs, the dim values of a pair side by side as in the walk.  anc = sum_c post[c][s] a_c
// (c ascending from 0.0); the thread of state 0 scans its pair's values in shared memory ascending and keeps the first index of the
// largest (-1 and 0.0 when none is above 0.0).  Every output entry has one writer; anc_post only when asked for.
struct PgmTreelikAncCombineArgs {
    uint32_t dim, ncat, ncols, spb;   // spb = 64 / dim
    uint64_t npairs, cat;             // (nnodes - nleaves) * ncols; doubles between two categories' posteriors
    const double *a, *post;           // ncat x npairs x dim; ncat x ncols
    double *anc_post, *anc_prob;      // npairs x dim or NULL; npairs
    int8_t *anc_state;                // npairs
};
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_anc_combine_kernel(PgmTreelikAncCombineArgs a) {
    __shared__ double sh[PGM_TREELIK_THREADS];
    const uint32_t dim = a.dim, local = threadIdx.x / dim, i = threadIdx.x - local * dim;
    for (uint64_t g0 = (uint64_t)blockIdx.x * a.spb; g0 < a.npairs; g0 += (uint64_t)gridDim.x * a.spb) {   // (uniform over the workgroup)
        const uint64_t g = g0 + local;
        const bool active = local < a.spb && g < a.npairs;
        if (active) {
            const size_t s = (size_t)(g % a.ncols), at = (size_t)g * dim + i;
            double anc = 0.0;
            for (uint32_t c = 0; c < a.ncat; ++c) anc = anc + a.post[(size_t)c * a.ncols + s] * a.a[a.cat * c + at];
            if (a.anc_post) a.anc_post[at] = anc;
            sh[threadIdx.x] = anc;
        }
        __syncthreads();
        if (active && i == 0) {
            int best = -1;
            double top = 0.0;
#pragma unroll 8
            for (uint32_t j = 0; j < dim; ++j) {
                const double x = sh[threadIdx.x + j];
                if (x > top) { top = x; best = (int)j; }
            }
            a.anc_state[g] = (int8_t)best;
            a.anc_prob[g] = top;
        }
        __syncthreads();   // (the scan's reads are done before the next round writes)
    }
}

// The nearest-neighbour interchanges of pgm_tree_nni scored from the stored pieces.  Candidate q = (v, a, c): a a
// child of v, c a child of u = parent[v] other than v; the neighbour tree has a and c exchanged.  A workgroup of PGM_TREELIK_NNI_WAVES
// wavefronts owns that many times 64 / dim consecutive sites, a wavefront's threads laid out per (site, state) as in the walk, and
// takes the candidates blockIdx.y, blockIdx.y + gridDim.y, ...; the categories run inside, ascending, so the mixture
// rho = sum_k post[k][s] rho_k needs no buffer.  Per category the thread of state i forms B_u(i), R(i), T(i), S_a(i), S_c(i) from global
// memory (the walk's sums: eight operands ahead of eight ordered adds), the four products X_D = T S_a, Y_D = R S_c, X_N = T S_c,
// Y_N = R S_a meet the scaling rule through shared memory together, W = P_v X reads the scaled X of its site from shared memory, and the
// thread of state 0 adds Y(i) W(i) over the states ascending for both trees and takes the ratio.  No workgroup waits for another, there
// are no atomics and every rho entry has one writer.  Every thread of the workgroup reaches every barrier: the loops over candidates,
// categories and children are uniform.
// EDGE (pgm_tree_nni_edge): the neighbour's W is formed three times, from P, P' and P'' of the candidate's own edge
// above v (n.Pc: [category][candidate][3] matrices, read from global memory as the walk reads an edge's three), the tree's own from
// P_v as before; four reductions (D, N, N', N'') through two more rows of shared memory; the thread of state 0 keeps rho, G and Q
// across the categories and writes rho and the per-site g = G / rho and h = Q / rho - g g, which pgm_treelik_sums_kernel adds per
// candidate.  The instantiation without EDGE is the kernel as it was: everything new stands behind `if constexpr (EDGE)`.
#define PGM_TREELIK_NNI_WAVES 4
#define PGM_TREELIK_NNI_THREADS (PGM_TREELIK_THREADS * PGM_TREELIK_NNI_WAVES)
struct PgmTreelikNniArgs {
    PgmTreelikArgs t;                      // the tree, rows, pi, and category 0's P, U, O (site_l, site_k, g, h unused)
    PgmTreelikRatesStride st;              // doubles between two categories' matrices (P) and partials (U)
    uint32_t ncat, ncand;
    const uint32_t *parent;                // nnodes
    const uint32_t *cand_v, *cand_a, *cand_c;
    const double *post;                    // ncat x ncols
    double *rho;                           // ncand x ncols
    const double *Pc;                      // EDGE: ncat x ncand x 3 x dim x dim
    double *g, *h;                         // EDGE: ncand x ncols each
};
template <bool EDGE>
__global__ __launch_bounds__(PGM_TREELIK_NNI_THREADS) void pgm_treelik_nni_kernel(PgmTreelikNniArgs n) {
    // 0 .. 3: the four products before scaling; 4, 5: X_D, X_N scaled; 6, 7: Y W of D, N; EDGE: 8, 9: Y W of N', N''
    __shared__ double sh[EDGE ? 10 : 8][PGM_TREELIK_NNI_THREADS];
    const uint32_t dim = n.t.dim, nleaves = n.t.nleaves, root = n.t.nnodes - 1, spb = n.t.spb, ncols = n.t.ncols;
    const uint32_t wave = threadIdx.x / PGM_TREELIK_THREADS, lane = threadIdx.x - wave * PGM_TREELIK_THREADS;
    const uint32_t local = lane / dim, i = lane - local * dim;
    const uint64_t s64 = ((uint64_t)blockIdx.x * PGM_TREELIK_NNI_WAVES + wave) * spb + local;
    const bool active = local < spb && s64 < ncols;
    const uint32_t s = (uint32_t)s64, first = threadIdx.x - i;   // first: the slot of this site's state 0
    const size_t mat = (size_t)dim * dim;

    for (uint32_t q = blockIdx.y; q < n.ncand; q += gridDim.y) {   // (uniform over the workgroup)
        const uint32_t v = n.cand_v[q], ca = n.cand_a[q], cc = n.cand_c[q], u = n.parent[v];
        const uint32_t u0 = n.t.child_off[u], u1 = n.t.child_off[u + 1], v0 = n.t.child_off[v], v1 = n.t.child_off[v + 1];
        double rho = 0.0, G = 0.0, Q = 0.0;   // (G, Q: EDGE only)
        for (uint32_t k = 0; k < n.ncat; ++k) {
            PgmTreelikArgs a = n.t;
            a.P += n.st.P * k;
            a.U += n.st.U * k;
            a.O += n.st.U * k;
            double XD = 0.0, YD = 0.0, XN = 0.0, YN = 0.0;
            if (active) {
                double R = 0.0;
                if (u == root) R = a.pi[i];
                else {
                    const double *o = a.O + ((size_t)(u - nleaves) * ncols + s) * dim, *Pu = a.P + mat * u + (size_t)dim * i;
                    uint32_t h = 0;
                    for (; h + 8 <= dim; h += 8) {
                        double ov[8], pv[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) { ov[e] = o[h + e]; pv[e] = Pu[h + e]; }
#pragma unroll
                        for (int e = 0; e < 8; ++e) R = R + ov[e] * pv[e];
                    }
                    for (; h < dim; ++h) R = R + o[h] * Pu[h];
                }
                double S[1];
                for (uint32_t r = u0; r < u1; ++r) {
                    const uint32_t sib = a.child[r];
                    if (sib == v || sib == cc) continue;
                    pgm_treelik_apply<1>(a, a.P + mat * sib, mat, sib, s, i, S);
                    R = R * S[0];
                }
                double T = 0.0;
                bool have = false;
                for (uint32_t r = v0; r < v1; ++r) {
                    const uint32_t b = a.child[r];
                    if (b == ca) continue;
                    pgm_treelik_apply<1>(a, a.P + mat * b, mat, b, s, i, S);
                    T = have ? T * S[0] : S[0];
                    have = true;
                }
                double Sa[1], Sc[1];
                pgm_treelik_apply<1>(a, a.P + mat * ca, mat, ca, s, i, Sa);
                pgm_treelik_apply<1>(a, a.P + mat * cc, mat, cc, s, i, Sc);
                XD = T * Sa[0]; YD = R * Sc[0]; XN = T * Sc[0]; YN = R * Sa[0];
                sh[0][threadIdx.x] = XD; sh[1][threadIdx.x] = YD; sh[2][threadIdx.x] = XN; sh[3][threadIdx.x] = YN;
            }
            __syncthreads();
            int32_t kD = 0, kN = 0;
            if (active) {   // the scaling rule on the four vectors of the site (every thread of the site finds the same maxima)
                double m0 = sh[0][first], m1 = sh[1][first], m2 = sh[2][first], m3 = sh[3][first];
#pragma unroll 8
                for (uint32_t j = 1; j < dim; ++j) {
                    const double x0 = sh[0][first + j], x1 = sh[1][first + j], x2 = sh[2][first + j], x3 = sh[3][first + j];
                    m0 = x0 > m0 ? x0 : m0; m1 = x1 > m1 ? x1 : m1; m2 = x2 > m2 ? x2 : m2; m3 = x3 > m3 ? x3 : m3;
                }
                if (m0 < 0x1p-256 && m0 > 0.0) { XD = XD * 0x1p256; ++kD; }
                if (m1 < 0x1p-256 && m1 > 0.0) { YD = YD * 0x1p256; ++kD; }
                if (m2 < 0x1p-256 && m2 > 0.0) { XN = XN * 0x1p256; ++kN; }
                if (m3 < 0x1p-256 && m3 > 0.0) { YN = YN * 0x1p256; ++kN; }
                sh[4][threadIdx.x] = XD; sh[5][threadIdx.x] = XN;
            }
            __syncthreads();
            if (active) {   // W(i) = sum_j P_v(i, j) X(j), then Y(i) W(i)
                const double *col = a.P + mat * v + i, *xd = &sh[4][first], *xn = &sh[5][first];
                double WD = 0.0, WN = 0.0;
                uint32_t j = 0;
                if constexpr (EDGE) {   // the neighbour's three sums from the candidate's own matrices, the tree's from P_v
                    const double *cz = n.Pc + ((size_t)k * n.ncand + q) * 3 * mat + i;
                    double W1 = 0.0, W2 = 0.0;
                    for (; j + 8 <= dim; j += 8) {
                        double pv[8], zv[3][8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            pv[e] = col[(size_t)dim * (j + e)];
#pragma unroll
                            for (int x = 0; x < 3; ++x) zv[x][e] = cz[mat * x + (size_t)dim * (j + e)];
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            WD = WD + pv[e] * xd[j + e];
                            WN = WN + zv[0][e] * xn[j + e]; W1 = W1 + zv[1][e] * xn[j + e]; W2 = W2 + zv[2][e] * xn[j + e];
                        }
                    }
                    for (; j < dim; ++j) {
                        const double pj = col[(size_t)dim * j], z0 = cz[(size_t)dim * j], z1 = cz[mat + (size_t)dim * j], z2 = cz[2 * mat + (size_t)dim * j];
                        WD = WD + pj * xd[j];
                        WN = WN + z0 * xn[j]; W1 = W1 + z1 * xn[j]; W2 = W2 + z2 * xn[j];
                    }
                    sh[8][threadIdx.x] = YN * W1; sh[9][threadIdx.x] = YN * W2;
                } else {
                    for (; j + 8 <= dim; j += 8) {
                        double pv[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) pv[e] = col[(size_t)dim * (j + e)];
#pragma unroll
                        for (int e = 0; e < 8; ++e) { WD = WD + pv[e] * xd[j + e]; WN = WN + pv[e] * xn[j + e]; }
                    }
                    for (; j < dim; ++j) { const double pj = col[(size_t)dim * j]; WD = WD + pj * xd[j]; WN = WN + pj * xn[j]; }
                }
                sh[6][threadIdx.x] = YD * WD; sh[7][threadIdx.x] = YN * WN;
            }
            __syncthreads();
            if (active && i == 0) {
                double D = 0.0, N = 0.0, N1 = 0.0, N2 = 0.0;
#pragma unroll 8
                for (uint32_t j = 0; j < dim; ++j) {
                    D = D + sh[6][threadIdx.x + j]; N = N + sh[7][threadIdx.x + j];
                    if constexpr (EDGE) { N1 = N1 + sh[8][threadIdx.x + j]; N2 = N2 + sh[9][threadIdx.x + j]; }
                }
                double r = 0.0, r1 = 0.0, r2 = 0.0;
                if (D != 0.0) {
                    r = N / D;
                    if constexpr (EDGE) { r1 = N1 / D; r2 = N2 / D; }
                    for (int32_t d = kN - kD; d > 0; --d) {
                        r = r * 0x1p-256;
                        if constexpr (EDGE) { r1 = r1 * 0x1p-256; r2 = r2 * 0x1p-256; }
                    }
                    for (int32_t d = kD - kN; d > 0; --d) {
                        r = r * 0x1p256;
                        if constexpr (EDGE) { r1 = r1 * 0x1p256; r2 = r2 * 0x1p256; }
                    }
                }
                const double pk = n.post[(size_t)k * ncols + s];
                rho = rho + pk * r;
                if constexpr (EDGE) { G = G + pk * r1; Q = Q + pk * r2; }
            }
            // (the next round writes sh[0 .. 3] only; sh[6 ..] are written again after two more barriers)
        }
        if (active && i == 0) {
            n.rho[(size_t)q * ncols + s] = rho;
            if constexpr (EDGE) {
                double g = 0.0, h = 0.0;
                if (rho != 0.0) { g = G / rho; h = Q / rho - g * g; }
                n.g[(size_t)q * ncols + s] = g;
                n.h[(size_t)q * ncols + s] = h;
            }
        }
    }
}

// Subtree pruning and regrafting scored from the stored pieces (pgm_tree_spr).  Candidate q = (v, y) with the path
// its C ABI side wrote (n.path: J, M, then a_0 = p .. a_J = a, c_1 .. c_M = y).  The layout is the NNI kernel's: a workgroup of
// PGM_TREELIK_NNI_WAVES wavefronts owns that many times 64 / dim consecutive sites, a thread per (site, state), and takes the
// candidates blockIdx.y, blockIdx.y + gridDim.y, ..; the categories run inside, ascending, the mixture in a register of the thread of
// state 0.  A workgroup recomputes the chain of its candidate: the two chain vectors (- without v, + with it) of a site live in shared
// memory, a thread holding its own state's values in registers; a step forms the next values from the scaled vectors (rows 2, 3),
// publishes them unscaled (rows 0, 1), and after a barrier every thread of the site finds the same maxima, scales its own values and
// publishes them (rows 2, 3) ahead of a second barrier.  Rows 4, 5 carry the terms of N and D to the thread of state 0.  The sums are
// the walk's: eight operands ahead of eight ordered adds.  No workgroup waits for another, there are no atomics, nothing is zeroed and
// every rho entry has one writer.  Every thread of the workgroup reaches every barrier: the loops over candidates, categories and path
// steps, and the branches on J and M, are uniform over the workgroup.
struct PgmTreelikSprArgs {
    PgmTreelikArgs t;                      // the tree, rows, pi, and category 0's P, U, O (site_l, site_k, g, h unused)
    PgmTreelikRatesStride st;              // doubles between two categories' matrices (P, Ph) and partials (U)
    uint32_t ncat, ncand, stride;          // stride: values per candidate in `path`
    const uint32_t *cand_v, *path;
    const double *Ph;                      // ncat x (nnodes - 1) x dim x dim
    const double *post;                    // ncat x ncols
    double *rho;                           // ncand x ncols
};

// am = sum over l ascending of X[step * l] * xm[l], ap the same with xp: X + i and step == dim for sum_l X(i, l) x(l), X + dim * i and
// step == 1 for sum_h x(h) X(h, i).  xm, xp: the site's vectors in shared memory.
__device__ __forceinline__ void pgm_treelik_spr_sum2(const double *X, size_t step, uint32_t dim, const double *xm, const double *xp, double &am, double &ap) {
    am = 0.0; ap = 0.0;
    uint32_t l = 0;
    for (; l + 8 <= dim; l += 8) {
        double pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pv[e] = X[step * (l + e)];
#pragma unroll
        for (int e = 0; e < 8; ++e) { am = am + pv[e] * xm[l + e]; ap = ap + pv[e] * xp[l + e]; }
    }
    for (; l < dim; ++l) { const double pl = X[step * l]; am = am + pl * xm[l]; ap = ap + pl * xp[l]; }
}
__device__ __forceinline__ double pgm_treelik_spr_sum1(const double *X, size_t step, uint32_t dim, const double *x) {
    double acc = 0.0;
    uint32_t l = 0;
    for (; l + 8 <= dim; l += 8) {
        double pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pv[e] = X[step * (l + e)];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = acc + pv[e] * x[l + e];
    }
    for (; l < dim; ++l) acc = acc + X[step * l] * x[l];
    return acc;
}
// the scaling rule on NV vectors of a site at once, a value of each per thread: unscaled through rows 0 .., scaled into rows 2 ..
// (what the next step reads).  Every thread of the workgroup calls it (two barriers).
template <int NV>
__device__ __forceinline__ void pgm_treelik_spr_rule(double (*sh)[PGM_TREELIK_NNI_THREADS], uint32_t dim, uint32_t first, bool active, double (&val)[NV], int32_t (&count)[NV]) {
    if (active) {
#pragma unroll
        for (int x = 0; x < NV; ++x) sh[x][threadIdx.x] = val[x];
    }
    __syncthreads();
    if (active) {
        double m[NV];
#pragma unroll
        for (int x = 0; x < NV; ++x) m[x] = sh[x][first];
#pragma unroll 8
        for (uint32_t j = 1; j < dim; ++j) {
#pragma unroll
            for (int x = 0; x < NV; ++x) { const double e = sh[x][first + j]; m[x] = e > m[x] ? e : m[x]; }
        }
#pragma unroll
        for (int x = 0; x < NV; ++x) {
            if (m[x] < 0x1p-256 && m[x] > 0.0) { val[x] = val[x] * 0x1p256; ++count[x]; }
            sh[2 + x][threadIdx.x] = val[x];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(PGM_TREELIK_NNI_THREADS) void pgm_treelik_spr_kernel(PgmTreelikSprArgs n) {
    __shared__ double sh[6][PGM_TREELIK_NNI_THREADS];
    const uint32_t dim = n.t.dim, nleaves = n.t.nleaves, root = n.t.nnodes - 1, spb = n.t.spb, ncols = n.t.ncols;
    const uint32_t wave = threadIdx.x / PGM_TREELIK_THREADS, lane = threadIdx.x - wave * PGM_TREELIK_THREADS;
    const uint32_t local = lane / dim, i = lane - local * dim;
    const uint64_t s64 = ((uint64_t)blockIdx.x * PGM_TREELIK_NNI_WAVES + wave) * spb + local;
    const bool active = local < spb && s64 < ncols;
    const uint32_t s = (uint32_t)s64, first = threadIdx.x - i;   // first: the slot of this site's state 0
    const size_t mat = (size_t)dim * dim;

    for (uint32_t q = blockIdx.y; q < n.ncand; q += gridDim.y) {   // (uniform over the workgroup)
        const uint32_t *path = n.path + (size_t)q * n.stride, *node = path + 2;
        const uint32_t J = path[0], M = path[1], v = n.cand_v[q], p = node[0], y = node[J + M];
        double rho = 0.0;
        for (uint32_t k = 0; k < n.ncat; ++k) {
            PgmTreelikArgs a = n.t;
            a.P += n.st.P * k;
            a.U += n.st.U * k;
            a.O += n.st.U * k;
            const double *Phy = n.Ph + n.st.P * k + mat * y;
            double e[2] = {0.0, 0.0}, Sv = 0.0, S[1];   // e: this thread's values of the - and the + chain vector
            int32_t cnt[2] = {0, 0};
            if (active) { pgm_treelik_apply<1>(a, a.P + mat * v, mat, v, s, i, S); Sv = S[0]; }
            if (J >= 1 || M == 0) {   // the chain start
                if (active) {
                    bool have = false;
                    for (uint32_t r = a.child_off[p]; r < a.child_off[p + 1]; ++r) {
                        const uint32_t c = a.child[r];
                        if (c == v) continue;
                        pgm_treelik_apply<1>(a, a.P + mat * c, mat, c, s, i, S);
                        e[0] = have ? e[0] * S[0] : S[0];
                        have = true;
                    }
                    e[1] = e[0] * Sv;
                }
                pgm_treelik_spr_rule<2>(sh, dim, first, active, e, cnt);
            }
            double mup[2] = {0.0, 0.0};
            for (uint32_t j = 1; j <= J; ++j) {   // up
                const uint32_t below = node[j - 1], at = node[j];
                if (active) pgm_treelik_spr_sum2(a.P + mat * below + i, dim, dim, &sh[2][first], &sh[3][first], mup[0], mup[1]);
                if (j < J || M == 0) {
                    if (active) {
                        e[0] = mup[0]; e[1] = mup[1];
                        for (uint32_t r = a.child_off[at]; r < a.child_off[at + 1]; ++r) {
                            const uint32_t c = a.child[r];
                            if (c == below) continue;
                            pgm_treelik_apply<1>(a, a.P + mat * c, mat, c, s, i, S);
                            e[0] = e[0] * S[0]; e[1] = e[1] * S[0];
                        }
                    }
                    pgm_treelik_spr_rule<2>(sh, dim, first, active, e, cnt);
                }
            }
            double tn = 0.0, td = 0.0;   // this state's terms of N and D
            if (M == 0) {   // the target on the up chain: y = a_J, an inner node below the root
                double X[1] = {0.0}, T = 0.0;
                if (active) {
                    X[0] = Sv * pgm_treelik_spr_sum1(Phy + i, dim, dim, &sh[2][first]);
                    T = pgm_treelik_spr_sum1(a.P + mat * y + i, dim, dim, &sh[3][first]);
                }
                int32_t c1[1] = {0};
                pgm_treelik_spr_rule<1>(sh, dim, first, active, X, c1);   // (scaled X into row 2: the sums above are done at its first barrier)
                cnt[0] += c1[0];
                if (active) {
                    const double W = pgm_treelik_spr_sum1(Phy + i, dim, dim, &sh[2][first]);
                    const double Oy = a.O[((size_t)(y - nleaves) * ncols + s) * dim + i];
                    tn = Oy * W; td = Oy * T;
                }
            } else {
                const uint32_t top = node[J], c_1 = node[J + 1];
                if (active) {   // the turn
                    double B = 0.0;
                    if (top == root) B = a.pi[i];
                    else {
                        const double *o = a.O + ((size_t)(top - nleaves) * ncols + s) * dim, *Pa = a.P + mat * top + (size_t)dim * i;
                        uint32_t h = 0;
                        for (; h + 8 <= dim; h += 8) {
                            double ov[8], pv[8];
#pragma unroll
                            for (int x = 0; x < 8; ++x) { ov[x] = o[h + x]; pv[x] = Pa[h + x]; }
#pragma unroll
                            for (int x = 0; x < 8; ++x) B = B + ov[x] * pv[x];
                        }
                        for (; h < dim; ++h) B = B + o[h] * Pa[h];
                    }
                    const uint32_t skip = J >= 1 ? node[J - 1] : v;
                    if (J >= 1) { e[0] = B * mup[0]; e[1] = B * mup[1]; }
                    else e[0] = B;
                    for (uint32_t r = a.child_off[top]; r < a.child_off[top + 1]; ++r) {
                        const uint32_t c = a.child[r];
                        if (c == skip || c == c_1) continue;
                        pgm_treelik_apply<1>(a, a.P + mat * c, mat, c, s, i, S);
                        e[0] = e[0] * S[0];
                        if (J >= 1) e[1] = e[1] * S[0];
                    }
                    if (J == 0) e[1] = e[0] * Sv;
                }
                pgm_treelik_spr_rule<2>(sh, dim, first, active, e, cnt);
                for (uint32_t m = 1; m < M; ++m) {   // down
                    const uint32_t at = node[J + m], next = node[J + m + 1];
                    if (active) {
                        pgm_treelik_spr_sum2(a.P + mat * at + (size_t)dim * i, 1, dim, &sh[2][first], &sh[3][first], e[0], e[1]);
                        for (uint32_t r = a.child_off[at]; r < a.child_off[at + 1]; ++r) {
                            const uint32_t c = a.child[r];
                            if (c == next) continue;
                            pgm_treelik_apply<1>(a, a.P + mat * c, mat, c, s, i, S);
                            e[0] = e[0] * S[0]; e[1] = e[1] * S[0];
                        }
                    }
                    pgm_treelik_spr_rule<2>(sh, dim, first, active, e, cnt);
                }
                double X[1] = {0.0}, Sy = 0.0;   // the target below the turn
                if (active) {
                    pgm_treelik_apply<1>(a, Phy, mat, y, s, i, S);
                    X[0] = Sv * S[0];
                    pgm_treelik_apply<1>(a, a.P + mat * y, mat, y, s, i, S);
                    Sy = S[0];
                }
                int32_t c1[1] = {0};
                pgm_treelik_spr_rule<1>(sh, dim, first, active, X, c1);
                cnt[0] += c1[0];
                if (active) {
                    const double W = pgm_treelik_spr_sum1(Phy + i, dim, dim, &sh[2][first]);
                    tn = e[0] * W; td = e[1] * Sy;
                }
            }
            if (active) { sh[4][threadIdx.x] = tn; sh[5][threadIdx.x] = td; }
            __syncthreads();
            if (active && i == 0) {
                double N = 0.0, D = 0.0;
#pragma unroll 8
                for (uint32_t j = 0; j < dim; ++j) { N = N + sh[4][threadIdx.x + j]; D = D + sh[5][threadIdx.x + j]; }
                double r = 0.0;
                if (D != 0.0) {
                    r = N / D;
                    for (int32_t d = cnt[0] - cnt[1]; d > 0; --d) r = r * 0x1p-256;
                    for (int32_t d = cnt[1] - cnt[0]; d > 0; --d) r = r * 0x1p256;
                }
                rho = rho + n.post[(size_t)k * ncols + s] * r;
            }
            // (rows 4, 5 are written again only after the barriers of the next round's target)
        }
        if (active && i == 0) n.rho[(size_t)q * ncols + s] = rho;
    }
}

// d1[e] = sum of g[e][.], d2[e] = sum of h[e][.]: sites ascending within chunks of PGM_TREELIK_CHUNK, then the chunk sums ascending.
// A workgroup per edge; chunk sums into `part` (nedges x 2 x nchunks), then thread 0 adds those of g and thread 1 those of h.
// pgm_tree_nni_edge runs it with its candidates in the place of the edges.
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_sums_kernel(const double *g, const double *h, uint32_t ncols, uint32_t nchunks, double *part,
                                                                                double *d1, double *d2) {
    const uint32_t e = blockIdx.x;
    const double *ge = g + (size_t)e * ncols, *he = h + (size_t)e * ncols;
    double *p1 = part + (size_t)e * 2 * nchunks, *p2 = p1 + nchunks;
    for (uint32_t chunk = threadIdx.x; chunk < nchunks; chunk += blockDim.x) {
        const uint32_t s0 = chunk * PGM_TREELIK_CHUNK, s1 = ncols - s0 < PGM_TREELIK_CHUNK ? ncols : s0 + PGM_TREELIK_CHUNK;
        double a1 = 0.0, a2 = 0.0;
        for (uint32_t s = s0; s < s1; ++s) { a1 = a1 + ge[s]; a2 = a2 + he[s]; }
        p1[chunk] = a1;
        p2[chunk] = a2;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *p = threadIdx.x == 0 ? p1 : p2;
        double acc = 0.0;
#pragma unroll 8
        for (uint32_t chunk = 0; chunk < nchunks; ++chunk) acc = acc + p[chunk];
        (threadIdx.x == 0 ? d1 : d2)[e] = acc;
    }
}

// The jointly most probable ancestral states (pgm_tree_ancestral_joint), after the walk (PGM_TREELIK_RAW without
// derivs) and the combine kernel gave post.  pgm_treelik_joint_kernel is the max-product up pass in the shape of the walk: a workgroup
// of one wavefront owns 64 / dim consecutive sites, a thread per (site, state), and goes over the inner nodes ascending.  The threads of
// a site find the site's category (the first of the largest post) themselves and read that category's matrices, so the sites of a
// workgroup may each read another category's; every loop and every barrier is uniform all the same.  At node v the thread of state i
// forms, per child c, m_c(i): the leaf rule of the walk, or max_j P_c(i, j) F_c(j) from the F the workgroup stored at c (eight
// operands fetched ahead of eight ordered compares), and writes the j that holds it as the back-pointer of (c, i): every node but the
// root has one parent, so a back-pointer has one writer.  The product of the m_c meets the scaling rule and goes to F.  The thread of
// state 0 then scans pi F_root.  The back-pointers lie [node][state][site], the sites fastest: pgm_treelik_joint_trace_kernel has a thread
// per site, 64 dependent chains in flight per wavefront, and its loads of one node run along the sites (different lanes read different
// state rows, each a run of the same 64 sites).  It goes over the nodes descending and finds the state of a node's parent in its own
// earlier write of joint_state.  No workgroup waits for another, nothing spins, there are no atomics and every entry has one writer.
struct PgmTreelikJointArgs {
    PgmTreelikArgs t;                      // the tree, rows, pi and category 0's P (U, O, g, h, site_l, site_k unused)
    size_t pstride;                        // doubles between two categories' matrices
    uint32_t ncat;
    const uint32_t *parent;                // nnodes
    const double *post;                    // ncat x ncols
    double *F;                             // ninner x ncols x dim
    uint8_t *ptr;                          // ninner x dim x ncols
    uint8_t *cat;                          // ncols
    int8_t *state;                         // ninner x ncols
    double *joint_l;                       // ncols
    int32_t *joint_k;                      // ncols
};
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_joint_kernel(PgmTreelikJointArgs n) {
    __shared__ double sh[PGM_TREELIK_THREADS];
    const PgmTreelikArgs &a = n.t;
    const uint32_t dim = a.dim, nleaves = a.nleaves, root = a.nnodes - 1, ncols = a.ncols;
    const uint32_t local = threadIdx.x / dim, i = threadIdx.x - local * dim;
    const uint64_t s64 = (uint64_t)blockIdx.x * a.spb + local;
    const bool active = local < a.spb && s64 < ncols;
    const uint32_t s = (uint32_t)s64;
    const size_t mat = (size_t)dim * dim;
    double *shs = &sh[local * dim];

    uint32_t k = 0;   // the site's category
    if (active) {
        double top = n.post[s];
        for (uint32_t c = 1; c < n.ncat; ++c) { const double x = n.post[(size_t)c * ncols + s]; if (x > top) { top = x; k = c; } }
    }
    const double *Pk = a.P + n.pstride * k;
    int32_t count = 0;
    for (uint32_t v = nleaves; v <= root; ++v) {
        double prod = 0.0;
        if (active) {
            const uint32_t q0 = a.child_off[v], q1 = a.child_off[v + 1];
            for (uint32_t q = q0; q < q1; ++q) {
                const uint32_t c = a.child[q];
                double m;
                if (c < nleaves) {
                    double S[1];
                    pgm_treelik_apply<1>(a, Pk + mat * c, mat, c, s, i, S);
                    m = S[0];
                } else {
                    const double *col = Pk + mat * c + i, *f = n.F + ((size_t)(c - nleaves) * ncols + s) * dim;
                    uint32_t arg = 0, j = 1;
                    m = col[0] * f[0];
                    for (; j + 8 <= dim; j += 8) {
                        double pv[8], fv[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) { pv[e] = col[(size_t)dim * (j + e)]; fv[e] = f[j + e]; }
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const double x = pv[e] * fv[e]; if (x > m) { m = x; arg = j + e; } }
                    }
                    for (; j < dim; ++j) { const double x = col[(size_t)dim * j] * f[j]; if (x > m) { m = x; arg = j; } }
                    n.ptr[((size_t)(c - nleaves) * dim + i) * ncols + s] = (uint8_t)arg;
                }
                prod = q == q0 ? m : prod * m;
            }
        }
        if (pgm_treelik_rescale(prod, shs, dim, i, active)) ++count;
        if (active) n.F[((size_t)(v - nleaves) * ncols + s) * dim + i] = prod;
        __syncthreads();   // the node's F is in memory before its parent reads it
    }
    if (active && i == 0) {
        const double *f = n.F + ((size_t)(root - nleaves) * ncols + s) * dim;
        double best = a.pi[0] * f[0];
        uint32_t arg = 0;
#pragma unroll 8
        for (uint32_t j = 1; j < dim; ++j) { const double x = a.pi[j] * f[j]; if (x > best) { best = x; arg = j; } }
        n.joint_l[s] = best;
        n.joint_k[s] = count;
        n.cat[s] = (uint8_t)k;
        n.state[(size_t)(root - nleaves) * ncols + s] = best == 0.0 ? (int8_t)-1 : (int8_t)arg;
    }
}
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_joint_trace_kernel(PgmTreelikJointArgs n) {
    const uint32_t dim = n.t.dim, nleaves = n.t.nleaves, root = n.t.nnodes - 1, ncols = n.t.ncols;
    const uint64_t s64 = (uint64_t)blockIdx.x * PGM_TREELIK_THREADS + threadIdx.x;
    if (s64 >= ncols) return;
    const size_t s = (size_t)s64;
    for (uint32_t v = root; v-- > nleaves;) {   // root - 1 down to nleaves: a parent's state is written before its children ask for it
        const int up = n.state[(size_t)(n.parent[v] - nleaves) * ncols + s];
        n.state[(size_t)(v - nleaves) * ncols + s] = up < 0 ? (int8_t)-1 : (int8_t)n.ptr[((size_t)(v - nleaves) * dim + (uint32_t)up) * ncols + s];
    }
}

// Ancestral states drawn from their joint posterior (pgm_tree_ancestral_sample), after the same walk and combine: the
// stochastic traceback through the stored partials.  A lane is a sample and a wavefront owns 64 consecutive samples of one site
// (blockIdx.x: the block of samples; the sites blockIdx.y, blockIdx.y + gridDim.y, ..), so the partial U_v(s, .) a node's draw reads is
// the same for the lanes of a category and the 64 bytes a node's draw writes are consecutive.  A lane draws its category, then the
// root, then the nodes descending, and finds the state of a node's parent in its own earlier write of samp_state.  Every draw has its
// own counter, so what a lane draws depends on (sample, site, node, seed) alone.  A weight is one multiply wherever it is read: the sum
// T and the running sum c form the same weights twice, eight fetched ahead of eight ordered adds.  No barriers, no atomics, one writer
// per entry.
struct PgmTreelikSampleArgs {
    PgmTreelikArgs t;                      // the tree, pi and category 0's P and U (the rest unused)
    PgmTreelikRatesStride st;              // doubles between two categories' matrices (P) and partials (U)
    uint32_t ncat, nsamp;
    uint64_t first, seed;
    const uint32_t *parent;                // nnodes
    const double *post;                    // ncat x ncols
    uint8_t *cat;                          // ncols x nsamp
    int8_t *state;                         // ninner x ncols x nsamp
};
// u of the draw numbered `counter`: splitmix64 (host/pgm_host.h) of the state seed + golden * counter, its top 53 bits times 2^-53
__device__ __forceinline__ double pgm_treelik_uniform(uint64_t seed, uint64_t counter) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * 0x1p-53;
}
// the pick rule of the interface on the weights weight(0) .. weight(m - 1)
template <class W>
__device__ __forceinline__ int pgm_treelik_pick(uint32_t m, double u, W weight) {
    double T = 0.0;
    uint32_t j = 0;
    for (; j + 8 <= m; j += 8) {
        double qv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = weight(j + e);
#pragma unroll
        for (int e = 0; e < 8; ++e) T = T + qv[e];
    }
    for (; j < m; ++j) T = T + weight(j);
    if (T == 0.0) return -1;
    const double target = u * T;
    double c = 0.0;
    int last = -1;
    for (j = 0; j + 8 <= m; j += 8) {
        double qv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = weight(j + e);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            c = c + qv[e];
            if (c > target) return (int)(j + e);
            if (qv[e] > 0.0) last = (int)(j + e);
        }
    }
    for (; j < m; ++j) {
        const double q = weight(j);
        c = c + q;
        if (c > target) return (int)j;
        if (q > 0.0) last = (int)j;
    }
    return last;
}
__global__ __launch_bounds__(PGM_TREELIK_THREADS) void pgm_treelik_sample_kernel(PgmTreelikSampleArgs n) {
    const uint32_t dim = n.t.dim, nleaves = n.t.nleaves, root = n.t.nnodes - 1, ncols = n.t.ncols, ninner = n.t.nnodes - nleaves;
    const uint64_t n64 = (uint64_t)blockIdx.x * PGM_TREELIK_THREADS + threadIdx.x;
    if (n64 >= n.nsamp) return;   // (no barrier below)
    const uint64_t N = n.first + n64;
    const size_t mat = (size_t)dim * dim, nsamp = n.nsamp, lane = (size_t)n64;
    const double *pi = n.t.pi;
    for (uint32_t s = blockIdx.y; s < ncols; s += gridDim.y) {
        const uint64_t base = (N * ncols + s) * ((uint64_t)ninner + 1);
        const double *post = n.post + s;
        const int k = pgm_treelik_pick(n.ncat, pgm_treelik_uniform(n.seed, base), [&](uint32_t c) { return post[(size_t)c * ncols]; });
        n.cat[(size_t)s * nsamp + lane] = (uint8_t)k;   // (-1: 255)
        const double *Pk = n.t.P + n.st.P * (size_t)(k < 0 ? 0 : k), *Uk = n.t.U + n.st.U * (size_t)(k < 0 ? 0 : k);
        int x = -1;
        if (k >= 0) {
            const double *u = Uk + ((size_t)(root - nleaves) * ncols + s) * dim;
            x = pgm_treelik_pick(dim, pgm_treelik_uniform(n.seed, base + 1 + (root - nleaves)), [&](uint32_t j) { return pi[j] * u[j]; });
        }
        n.state[((size_t)(root - nleaves) * ncols + s) * nsamp + lane] = (int8_t)x;
        for (uint32_t v = root; v-- > nleaves;) {   // root - 1 down to nleaves, parents first
            const int up = n.state[((size_t)(n.parent[v] - nleaves) * ncols + s) * nsamp + lane];
            x = -1;
            if (up >= 0) {   // (then k >= 0)
                const double *row = Pk + mat * v + (uint32_t)up, *u = Uk + ((size_t)(v - nleaves) * ncols + s) * dim;
                x = pgm_treelik_pick(dim, pgm_treelik_uniform(n.seed, base + 1 + (v - nleaves)), [&](uint32_t j) { return row[(size_t)dim * j] * u[j]; });
            }
            n.state[((size_t)(v - nleaves) * ncols + s) * nsamp + lane] = (int8_t)x;
        }
    }
}

#endif
