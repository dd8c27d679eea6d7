// pgm_dist_kernels.h — the tail of the guide-tree stages on the GPU:
//   pgm_mldist_kernel      DistanceFactoryML::computeDistance + computeMLDist (reference src/DistanceFactoryML.h:66-190),
//                          one wavefront per sequence pair: bracketed Newton iteration on the distance d, every step a
//                          20 x 20 P(d) = V diag(exp(sigma d)) V^-1, Q P, Q Q P and two sums over the 400 pair counts
//   pgm_mldist_general_kernel  the same estimator for a generator without an eigen form or with up to 64 states (the 61-state
//                          codon model): one workgroup per pair, P(d) = exp(Q d) by the host's scaling-and-squaring expm
//   pgm_prealigned_kernel  DistanceFactoryPrealigned::computePwDistances' pair counts (src/DistanceFactoryPrealigned.h:34-90):
//                          residue-pair counts and gap openings of every pair of rows of an alignment
// fp64 throughout.  Every sum keeps the host mirror's order (host/mldist.cpp, host/model_factory.cpp): matrix
// products accumulate k = 0..n-1 from zero with one multiply and one add per term (no FMA), the two sums over the
// count matrix run over the entries in storage order.  What is NOT bit-identical to the host is exp() (and one log()):
// the device library's results can differ from glibc's in the last bit, so distances agree to ~1e-15 relative, not
// always to the bit (tests/test_gpu_dist.py: 1e-12).
#ifndef PGM_DIST_KERNELS_H_
#define PGM_DIST_KERNELS_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

struct PgmMlArgs {
    uint32_t dim, npairs;
    const double *Q, *V, *Vi, *sigma;   // dim x dim column-major (Q, V, V^-1), dim eigenvalues
    const int32_t *counts;              // npairs x dim x dim
    const uint32_t *gaps;               // npairs
    const double *seqlen;               // npairs: (L1 + L2) / 2
    double dist_max, var_max, var_min, cutoff_dist, min_dist, max_dist, indel_rate;
    int mldist, mldist_gap;
    double *dist, *var;                 // npairs each
};

#define PGM_ML_WAVES 4
#define PGM_ML_DMAX 20

// The estimator around the two sums, shared by the two kernels below: computeDistance's start value (DistanceFactoryML.h:137-190),
// computeMLDist's bracketed Newton iteration with its MAXITER exit and the -M gap term (:66-135), the final clamps.  ident / total
// are integer sums (exact in fp64 whatever the order).  sums(dm, f, ff) evaluates f = sum c P'/P and f' = sum c (P'' P - P'^2) / P^2
// at the clamped distance dm (getModel(dist): parseDistance, ModelFactory.h:104-127); every thread that runs the estimator together
// must get the same f and f' from it, so that the control flow here is uniform over them.
template <class Sums>
__device__ __forceinline__ void pgm_ml_estimate(const PgmMlArgs &A, long long ident, long long total, double gapsd, double seqlen, Sums sums,
                                                double &dist_out, double &var_out) {
    const double identd = (double)ident, totald = (double)total;
    double dist0 = __dsub_rn(1.0, __ddiv_rn(identd, totald));
    double dist, var;
    if (A.mldist || A.mldist_gap) {
        if (total == 0 || dist0 > 0.85) { dist = dist0 = A.dist_max; var = A.var_max; }
        else {
            dist = dist0 = -log(__dsub_rn(__dsub_rn(1.0, dist0), __dmul_rn(__dmul_rn(0.2, dist0), dist0)));
            var = __ddiv_rn(dist, totald);
        }
        if (total > 0 && ident != total) {
            // computeMLDist (DistanceFactoryML.h:66-135)
            const double var0 = var;
            double dist_min = 0.0, dist_maxb = INFINITY, delta = 1.0;
            int iteration = 0;
            while (fabs(delta) > 1e-5) {
                if (iteration > 20) {
                    if (dist_maxb == INFINITY) { dist = A.dist_max; var = A.var_max; }
                    else { dist = dist0; var = var0; }
                    break;
                }
                double dm = fmax(0.0, dist);
                if (dist != dist) dm = 5.2;
                dm = fmax(fmin(dm, A.max_dist), A.min_dist);
                double f, ff;
                sums(dm, f, ff);
                if (A.mldist_gap) {
                    const double grate = __dmul_rn(__dmul_rn(A.indel_rate, seqlen), dist);
                    f = __dadd_rn(f, __ddiv_rn(__dadd_rn(-grate, gapsd), dist));
                    ff = __dadd_rn(ff, -__ddiv_rn(gapsd, __dmul_rn(dist, dist)));
                }
                var = __ddiv_rn(-1.0, ff);
                if (f > 0) dist_min = fmax(dist_min, dist); else dist_maxb = fmin(dist_maxb, dist);
                double new_dist = __dsub_rn(dist, __ddiv_rn(f, ff));
                if (!(new_dist < dist_maxb && new_dist > dist_min)) {
                    const double upper = (dist_maxb == INFINITY) ? __dmul_rn(dist, 3.0) : dist_maxb;
                    new_dist = __ddiv_rn(__dadd_rn(upper, dist_min), 2.0);
                }
                delta = __dsub_rn(1.0, __ddiv_rn(new_dist, dist));
                dist = new_dist;
                ++iteration;
            }
        }
    } else {
        if (total == 0) { dist = dist0 = 1.0; var = A.var_max; }
        else { dist = dist0; var = __ddiv_rn(dist0, totald); }
    }
    if (!(dist < A.dist_max)) { dist = A.dist_max; var = A.var_max; }
    if (dist > A.cutoff_dist) dist = A.cutoff_dist;
    if (var < A.var_min) var = A.var_min;
    if (!(var < A.var_max)) var = A.var_max;
    dist_out = dist; var_out = var;
}

// One wavefront per pair; lane l owns the matrix entries e = l, l + 64, ... (entry e = i + n j, column-major like the host).
__global__ void __launch_bounds__(PGM_ML_WAVES * 64) pgm_mldist_kernel(PgmMlArgs A) {
    constexpr int N = PGM_ML_DMAX, NN = N * N, EPL = (NN + 63) / 64;
    __shared__ double sQ[NN], sV[NN], sVi[NN], sSig[N];
    __shared__ double sE[PGM_ML_WAVES][N], sP[PGM_ML_WAVES][NN], sPP[PGM_ML_WAVES][NN], sT1[PGM_ML_WAVES][NN], sT2[PGM_ML_WAVES][NN];
    const int n = (int)A.dim, nn = n * n;
    for (int i = threadIdx.x; i < nn; i += PGM_ML_WAVES * 64) { sQ[i] = A.Q[i]; sV[i] = A.V[i]; sVi[i] = A.Vi[i]; }
    for (int i = threadIdx.x; i < n; i += PGM_ML_WAVES * 64) sSig[i] = A.sigma[i];
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *E = sE[w], *P = sP[w], *PP = sPP[w], *T1 = sT1[w], *T2 = sT2[w];
    for (uint32_t pair = blockIdx.x * PGM_ML_WAVES + w; pair < A.npairs; pair += gridDim.x * PGM_ML_WAVES) {
        const int32_t *cnt = A.counts + (size_t)pair * nn;
        long long ident = 0, total = 0;
        for (int e = lane; e < nn; e += 64) {
            const int c = cnt[e];
            total += c;
            if (e % n == e / n) ident += c;
        }
        for (int o = 32; o > 0; o >>= 1) { ident += __shfl_xor(ident, o); total += __shfl_xor(total, o); }
        // P = V diag(exp(sigma d)) V^-1, Q P, Q Q P and the two sums
        auto sums = [&](double dm, double &f, double &ff) {
            if (lane < n) E[lane] = exp(__dmul_rn(sSig[lane], dm));
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                const int e = lane + 64 * u;
                if (e < nn) {
                    const int i = e % n, j = e / n;
                    double acc = 0.0;
                    for (int k = 0; k < n; ++k) acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(sV[i + n * k], E[k]), sVi[k + n * j]));
                    P[e] = acc;
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                const int e = lane + 64 * u;
                if (e < nn) {
                    const int i = e % n, j = e / n;
                    double acc = 0.0;
                    for (int k = 0; k < n; ++k) acc = __dadd_rn(acc, __dmul_rn(sQ[i + n * k], P[k + n * j]));
                    PP[e] = acc;
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                const int e = lane + 64 * u;
                if (e < nn) {
                    const int i = e % n, j = e / n;
                    double ppp = 0.0;
                    for (int k = 0; k < n; ++k) ppp = __dadd_rn(ppp, __dmul_rn(sQ[i + n * k], PP[k + n * j]));
                    const double c = (double)cnt[e], p = P[e], pp = PP[e];
                    T1[e] = __ddiv_rn(__dmul_rn(c, pp), p);
                    T2[e] = __ddiv_rn(__dmul_rn(c, __dsub_rn(__dmul_rn(ppp, p), __dmul_rn(pp, pp))), __dmul_rn(p, p));
                }
            }
            __builtin_amdgcn_wave_barrier();
            // the two sums run over the entries in storage order (every lane adds the same 400 terms: uniform result)
            f = 0.0; ff = 0.0;
            for (int e = 0; e < nn; ++e) { f = __dadd_rn(f, T1[e]); ff = __dadd_rn(ff, T2[e]); }
            __builtin_amdgcn_wave_barrier();
        };
        double dist, var;
        pgm_ml_estimate(A, ident, total, (double)A.gaps[pair], A.seqlen[pair], sums, dist, var);
        if (lane == 0) { A.dist[pair] = dist; A.var[pair] = var; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same estimator for a general generator Q (dim <= 64, no eigen form: the 61-state ECM codon model, any generator that is
// not reversible).  P(d) = exp(Q d) is the host's expm (host/model_factory.cpp) step by step: A = Q d scaled by 2^-s with s from
// the 1-norm rule (||A / 2^s||_1 <= 1/2), 20 Taylor terms term = term A / k added to E in that order, s squarings; then Q P,
// Q Q P and the two sums in storage order.  Every product keeps the host matmul's association: k ascending from zero, one
// multiply and one add per term.
// One workgroup of 256 threads per pair.  A thread owns a 4 x 4 register tile of every matrix: rows 2 ti + {0, 1} + 32 {0, 1},
// columns tj + 16 {0 .. 3} (ti = t % 16, tj = t / 16), so a step of k reads 4 + 4 operands from LDS for 16 multiply-adds.  E,
// P, Q P and the counts stay in registers; LDS holds Q and the two operands of the running product, column-major with the
// stride PGM_MLG_LD = 66 doubles: even, so that a thread's two rows are one aligned 16-byte read and the 16 lanes of a
// column read 256 contiguous bytes; and 132 dwords = 4 mod 64, so that the columns tj, tj + 1, ... a wavefront reads of
// the right operand start in different banks (a dense 64-wide column would put them all into one).  Rows and columns from dim on
// are zero in all three matrices and are never written, so the products need no bounds in the inner loop.
#define PGM_MLG_DMAX 64
#define PGM_MLG_LD 66
#define PGM_MLG_THREADS 256

struct PgmMlgTile { double v[4][4]; };

__device__ __forceinline__ int pgm_mlg_row(int ti, int a) { return 2 * ti + (a & 1) + 32 * (a >> 1); }
__device__ __forceinline__ int pgm_mlg_col(int tj, int b) { return tj + 16 * b; }

// C = X Y on the thread's tile
__device__ __forceinline__ void pgm_mlg_matmul(const double *__restrict__ X, const double *__restrict__ Y, int n, int ti, int tj, PgmMlgTile &C) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) C.v[a][b] = 0.0;
    const double *x = X + 2 * ti, *y = Y + PGM_MLG_LD * tj;
#pragma unroll 2
    for (int k = 0; k < n; ++k) {
        const double2 x0 = *reinterpret_cast<const double2 *>(x + PGM_MLG_LD * k), x1 = *reinterpret_cast<const double2 *>(x + PGM_MLG_LD * k + 32);
        const double xv[4] = {x0.x, x0.y, x1.x, x1.y};
        double yv[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) yv[b] = y[k + 16 * PGM_MLG_LD * b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) C.v[a][b] = __dadd_rn(C.v[a][b], __dmul_rn(xv[a], yv[b]));
    }
}

// the entries of the tile inside the dim x dim matrix go to M (the rest of M stays zero)
__device__ __forceinline__ void pgm_mlg_store(double *__restrict__ M, int n, int ti, int tj, const PgmMlgTile &C) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = pgm_mlg_row(ti, a), j = pgm_mlg_col(tj, b);
            if (i < n && j < n) M[i + PGM_MLG_LD * j] = C.v[a][b];
        }
}

__global__ void __launch_bounds__(PGM_MLG_THREADS) pgm_mldist_general_kernel(PgmMlArgs A) {
    constexpr int LD = PGM_MLG_LD, SZ = PGM_MLG_LD * PGM_MLG_DMAX;
    __shared__ __attribute__((aligned(16))) double sQ[SZ], sA[SZ], sT[SZ];
    __shared__ double sNorm[PGM_MLG_DMAX], sSum[2];
    __shared__ long long sCnt[2 * PGM_MLG_THREADS / 64];
    const int n = (int)A.dim, nn = n * n, t = (int)threadIdx.x, ti = t & 15, tj = t >> 4;
    const uint32_t pair = blockIdx.x;
    if (pair >= A.npairs) return;
    for (int e = t; e < SZ; e += PGM_MLG_THREADS) { sQ[e] = 0.0; sA[e] = 0.0; sT[e] = 0.0; }
    __syncthreads();
    for (int e = t; e < nn; e += PGM_MLG_THREADS) sQ[e % n + LD * (e / n)] = A.Q[e];
    // the thread's counts; ident / total over the workgroup
    const int32_t *cnt = A.counts + (size_t)pair * nn;
    PgmMlgTile c;
    long long ident = 0, total = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = pgm_mlg_row(ti, a), j = pgm_mlg_col(tj, b);
            const int v = (i < n && j < n) ? cnt[i + n * j] : 0;
            c.v[a][b] = (double)v;
            total += v;
            if (i == j) ident += v;
        }
    for (int o = 32; o > 0; o >>= 1) { ident += __shfl_xor(ident, o); total += __shfl_xor(total, o); }
    if ((t & 63) == 0) { sCnt[2 * (t >> 6)] = ident; sCnt[2 * (t >> 6) + 1] = total; }
    __syncthreads();
    ident = 0; total = 0;
    for (int w = 0; w < PGM_MLG_THREADS / 64; ++w) { ident += sCnt[2 * w]; total += sCnt[2 * w + 1]; }

    // f and f' at the distance dm.  Every thread ends with the same two sums (one wavefront adds them, all read them from
    // LDS), so the Newton control flow around the barriers in here is uniform over the workgroup.
    auto sums = [&](double dm, double &f, double &ff) {
        // expm's scaling: the 1-norm of A = Q dm (the largest column sum of |A|, rows ascending), halved until it is <= 1/2
        if (t < n) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s = __dadd_rn(s, fabs(__dmul_rn(sQ[i + LD * t], dm)));
            sNorm[t] = s;
        }
        __syncthreads();
        double norm = 0.0;
        for (int j = 0; j < n; ++j) norm = fmax(norm, sNorm[j]);
        int sq = 0;
        while (norm > 0.5 && sq < 1100) { norm = __dmul_rn(norm, 0.5); ++sq; }   // (a finite norm is there after at most 1075 halvings: the cap only ends the loop for an infinite one)
        const double scale = ldexp(1.0, -sq);
        PgmMlgTile E, term, acc;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = pgm_mlg_row(ti, a), j = pgm_mlg_col(tj, b);
                const bool in = i < n && j < n;
                E.v[a][b] = (in && i == j) ? 1.0 : 0.0;
                if (in) {
                    sA[i + LD * j] = __dmul_rn(__dmul_rn(sQ[i + LD * j], dm), scale);
                    sT[i + LD * j] = E.v[a][b];
                }
            }
        __syncthreads();
        for (int k = 1; k <= 20; ++k) {
            pgm_mlg_matmul(sT, sA, n, ti, tj, acc);
            const double inv = __ddiv_rn(1.0, (double)k);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    term.v[a][b] = __dmul_rn(acc.v[a][b], inv);
                    E.v[a][b] = __dadd_rn(E.v[a][b], term.v[a][b]);
                }
            __syncthreads();                      // every thread has read the old term
            pgm_mlg_store(sT, n, ti, tj, k < 20 ? term : E);   // (after the last term: E, the operand of the squarings)
            __syncthreads();
        }
        for (int q = 0; q < sq; ++q) {
            pgm_mlg_matmul(sT, sT, n, ti, tj, E);
            __syncthreads();
            pgm_mlg_store(sT, n, ti, tj, E);
            __syncthreads();
        }
        // P = E (registers and sT); P' = Q P -> sA; P'' = Q P'
        PgmMlgTile pp;
        pgm_mlg_matmul(sQ, sT, n, ti, tj, pp);
        pgm_mlg_store(sA, n, ti, tj, pp);         // (nothing reads sA between the last Taylor product and here)
        __syncthreads();
        pgm_mlg_matmul(sQ, sA, n, ti, tj, acc);   // P''
        __syncthreads();
        // the terms of the two sums, at their entries: sT <- c P' / P, sA <- c (P'' P - P'^2) / P^2
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = pgm_mlg_row(ti, a), j = pgm_mlg_col(tj, b);
                if (i < n && j < n) {
                    const double cc = c.v[a][b], p = E.v[a][b], p1 = pp.v[a][b], p2 = acc.v[a][b];
                    sT[i + LD * j] = __ddiv_rn(__dmul_rn(cc, p1), p);
                    sA[i + LD * j] = __ddiv_rn(__dmul_rn(cc, __dsub_rn(__dmul_rn(p2, p), __dmul_rn(p1, p1))), __dmul_rn(p, p));
                }
            }
        __syncthreads();
        // storage order: columns ascending, rows ascending within a column.  The first wavefront adds (its lanes all the same
        // terms), the workgroup reads the two sums from LDS: the same bits in every thread
        if (t < 64) {
            double f0 = 0.0, f1 = 0.0;
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i) { f0 = __dadd_rn(f0, sT[i + LD * j]); f1 = __dadd_rn(f1, sA[i + LD * j]); }
            if (t == 0) { sSum[0] = f0; sSum[1] = f1; }
        }
        __syncthreads();
        f = sSum[0]; ff = sSum[1];
    };
    double dist, var;
    pgm_ml_estimate(A, ident, total, (double)A.gaps[pair], A.seqlen[pair], sums, dist, var);
    if (t == 0) { A.dist[pair] = dist; A.var[pair] = var; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Pair counts of an alignment.  rows: nrows x ncols int8, row-major: residue value() 0..dim-1, -1 = gap, -2 = a residue
// without a value (unknown: it is a residue for the gap bookkeeping, but never counted).  Only values < 20 are counted,
// for every alphabet (the reference's literal 20, DistanceFactoryPrealigned.h).  One wavefront per pair: lane l scans the
// columns [l * chunk, (l + 1) * chunk); the gap openings of the state machine (a run in which exactly one row has a
// residue opens one gap; columns where both rows have a gap are skipped) are counted per chunk with "no run open" at the
// chunk's start and corrected at the chunk boundaries afterwards.
struct PgmPaArgs {
    uint32_t dim, nrows, ncols, npairs;
    const int8_t *rows;
    const uint32_t *pi, *pj;
    int32_t *counts;     // npairs x dim x dim, zero-initialised
    uint32_t *gaps;      // npairs
};

// Which column of the stored rows column k of the scanned alignment is: itself, or cols[k] (a bootstrap replicate: the alignment
// with its columns gathered in that order; pgm_prealigned_resampled_kernel)
struct PgmPaColSelf { __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return k; } };
struct PgmPaColGather {
    const uint32_t *__restrict__ cols;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return cols[k]; }
};

// one pair on one wavefront: rows r1, r2 of L columns; cnt: the wavefront's 400 LDS counters
template <class Col>
__device__ __forceinline__ void pgm_prealigned_pair(const int8_t *__restrict__ r1, const int8_t *__restrict__ r2, uint32_t L, uint32_t D, int *cnt,
                                                    int32_t *__restrict__ out, uint32_t *__restrict__ gaps_out, int lane, Col col) {
    const uint32_t chunk = (L + 63u) / 64u;
    for (int i = lane; i < 400; i += 64) cnt[i] = 0;
    __builtin_amdgcn_wave_barrier();
    // type of a column: 0 both residues, 1 only row 1 has a residue, 2 only row 2, 3 both gaps (skipped)
    int first = 3, last = 3;
    uint32_t g = 0;
    const uint32_t k0 = min(L, (uint32_t)lane * chunk), k1 = min(L, k0 + chunk);
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t src = col(k);
        const int c1 = r1[src], c2 = r2[src];
        const bool g1 = c1 == -1, g2 = c2 == -1;
        const int ty = (!g1 && !g2) ? 0 : ((g1 && g2) ? 3 : (!g1 ? 1 : 2));
        if (ty == 3) continue;
        if (ty == 0) { if (c1 >= 0 && c1 < 20 && c2 >= 0 && c2 < 20) atomicAdd(&cnt[c1 + 20 * c2], 1); }
        else if (ty != last) ++g;            // a run opens (the previous non-skipped column was of another type)
        if (first == 3) first = ty;
        last = ty;
    }
    // chunk boundaries: a chunk whose first non-skipped column continues the run the previous non-empty chunk ended in
    // has counted one opening too many
    int prev_last = 3;
    uint32_t total = 0;
    for (int l = 0; l < 64; ++l) {
        const int f = __builtin_amdgcn_readlane(first, l), la = __builtin_amdgcn_readlane(last, l);
        total += (uint32_t)__builtin_amdgcn_readlane((int)g, l);
        if (f != 3) {
            if (f != 0 && f == prev_last) --total;
            prev_last = la;
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < 400; i += 64) {
        const int c1 = i % 20, c2 = i / 20;
        if ((uint32_t)c1 < D && (uint32_t)c2 < D) out[c1 + D * c2] = cnt[i];
    }
    if (lane == 0) *gaps_out = total;
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256) pgm_prealigned_kernel(PgmPaArgs A) {
    __shared__ int cnt[4][400];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t D = A.dim, L = A.ncols;
    for (uint32_t pair = blockIdx.x * 4 + w; pair < A.npairs; pair += gridDim.x * 4)
        pgm_prealigned_pair(A.rows + (size_t)A.pi[pair] * L, A.rows + (size_t)A.pj[pair] * L, L, D, cnt[w], A.counts + (size_t)pair * D * D, A.gaps + pair, lane, PgmPaColSelf());
}

// The same for the alignments of many families in one launch (pgm_prealigned_counts_multi): pair p compares rows pi[p], pj[p] of
// family fam[p], whose matrix starts at rows + base[fam[p]] and has ncols[fam[p]] columns.  The per-pair code is the one above.
struct PgmPaMultiArgs {
    uint32_t dim, npairs;
    const int8_t *rows;
    const uint64_t *base;     // per family: offset of its matrix in rows
    const uint32_t *ncols;    // per family
    const uint32_t *fam, *pi, *pj;
    int32_t *counts;          // npairs x dim x dim, zero-initialised
    uint32_t *gaps;           // npairs
};

__global__ void __launch_bounds__(256) pgm_prealigned_multi_kernel(PgmPaMultiArgs A) {
    __shared__ int cnt[4][400];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t D = A.dim;
    for (uint32_t pair = blockIdx.x * 4 + w; pair < A.npairs; pair += gridDim.x * 4) {
        const uint32_t f = A.fam[pair], L = A.ncols[f];
        const int8_t *m = A.rows + A.base[f];
        pgm_prealigned_pair(m + (size_t)A.pi[pair] * L, m + (size_t)A.pj[pair] * L, L, D, cnt[w], A.counts + (size_t)pair * D * D, A.gaps + pair, lane, PgmPaColSelf());
    }
}

// The same for nrep resamplings of the columns of one alignment (pgm_prealigned_counts_resampled): replicate r is the alignment whose
// column k is the stored column cols[r * ncols + k], and its pair p writes counts[r * npairs + p] and gaps[r * npairs + p].  The grid
// is (blocks of 4 pairs, replicates); the per-pair code is the one above with the column read through cols, so the gap openings are
// those of the gathered matrix.  The rows are stored once and read in place: a wavefront's two rows (ncols bytes each, any ncols)
// have no fixed place in the 4 x 400 counters' LDS layout, and its reads of them, in the order cols gives, stay within those
// 2 ncols bytes, which the caches hold.
struct PgmPaResampledArgs {
    uint32_t dim, ncols, npairs, nrep;
    const int8_t *rows;
    const uint32_t *cols;     // nrep x ncols, every entry < ncols
    const uint32_t *pi, *pj;
    int32_t *counts;          // nrep x npairs x dim x dim, zero-initialised
    uint32_t *gaps;           // nrep x npairs
};

__global__ void __launch_bounds__(256) pgm_prealigned_resampled_kernel(PgmPaResampledArgs A) {
    __shared__ int cnt[4][400];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t D = A.dim, L = A.ncols;
    for (uint32_t rep = blockIdx.y; rep < A.nrep; rep += gridDim.y) {
        const PgmPaColGather col{A.cols + (size_t)rep * L};
        for (uint32_t pair = blockIdx.x * 4 + w; pair < A.npairs; pair += gridDim.x * 4) {
            const size_t o = (size_t)rep * A.npairs + pair;
            pgm_prealigned_pair(A.rows + (size_t)A.pi[pair] * L, A.rows + (size_t)A.pj[pair] * L, L, D, cnt[w], A.counts + o * D * D, A.gaps + o, lane, col);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k-mer cosine matrix of DistanceFactoryAngle (reference src/DistanceFactoryAngle.h:55-115): the one dense
// contraction of the program.  counts: nseq x ncols int32 (row i = the k-mer counts of sequence i, ncols = DIM^K: 400 for amino
// acids, 3721 for codons).  The reference evaluates diag(1/|c_i|) * C * C^T * diag(1/|c_j|) left to right in double:
//     out(i, j) = (sum_k (c_ik * inv_i) * c_jk) * inv_j,     inv_i = 1 / sqrt(sum_k c_ik^2)
// k ascending, one fp64 multiply and one add per term (no FMA), in depth blocks of `kc` terms whose sums are added to the result
// one after the other: Eigen's GEMM (kc = L1d / 128 terms, 384 on the golden files' host; include/pgm_hip.h).  The norms are
// exact (integer sums of squares, correctly rounded sqrt and reciprocal).  One thread per (i, j), 16 x 16 outputs per workgroup, the two 16-row slabs staged through LDS in
// chunks of 64 columns (the i-slab already scaled).
#define PGM_KC_TILE 16
#define PGM_KC_CHUNK 64
// the 16 x 16 tile (by, bx) of one nseq x nseq matrix
__device__ __forceinline__ void pgm_kmer_cosine_tile(uint32_t nseq, uint32_t ncols, const int32_t *__restrict__ counts, const double *__restrict__ inv_norm,
                                                     double *__restrict__ out, uint32_t kc, uint32_t bx, uint32_t by,
                                                     double (*sa)[PGM_KC_CHUNK + 1], double (*sb)[PGM_KC_CHUNK + 1]) {
    const uint32_t tx = threadIdx.x % PGM_KC_TILE, ty = threadIdx.x / PGM_KC_TILE;
    const uint32_t i = by * PGM_KC_TILE + ty, j = bx * PGM_KC_TILE + tx;
    double acc = 0.0, res = 0.0;
    uint32_t left = kc;   // terms left in the depth block
    for (uint32_t k0 = 0; k0 < ncols; k0 += PGM_KC_CHUNK) {
        for (uint32_t e = threadIdx.x; e < PGM_KC_TILE * PGM_KC_CHUNK; e += PGM_KC_TILE * PGM_KC_TILE) {
            const uint32_t r = e / PGM_KC_CHUNK, c = e % PGM_KC_CHUNK, k = k0 + c;
            const uint32_t ri = by * PGM_KC_TILE + r, rj = bx * PGM_KC_TILE + r;
            sa[r][c] = (ri < nseq && k < ncols) ? __dmul_rn((double)counts[(size_t)ri * ncols + k], inv_norm[ri]) : 0.0;
            sb[r][c] = (rj < nseq && k < ncols) ? (double)counts[(size_t)rj * ncols + k] : 0.0;
        }
        __syncthreads();
        const uint32_t kn = min((uint32_t)PGM_KC_CHUNK, ncols - k0);
        for (uint32_t c = 0; c < kn; ++c) {
            acc = __dadd_rn(acc, __dmul_rn(sa[ty][c], sb[tx][c]));
            if (--left == 0u) { res = __dadd_rn(res, acc); acc = 0.0; left = kc; }
        }
        __syncthreads();
    }
    if (left != kc) res = __dadd_rn(res, acc);   // the last, shorter block
    if (i < nseq && j < nseq) out[(size_t)i + (size_t)nseq * j] = __dmul_rn(res, inv_norm[j]);
}
__global__ void __launch_bounds__(PGM_KC_TILE * PGM_KC_TILE) pgm_kmer_cosine_kernel(uint32_t nseq, uint32_t ncols, const int32_t *__restrict__ counts,
                                                                                 const double *__restrict__ inv_norm, double *__restrict__ out, uint32_t kc) {
    __shared__ double sa[PGM_KC_TILE][PGM_KC_CHUNK + 1], sb[PGM_KC_TILE][PGM_KC_CHUNK + 1];
    pgm_kmer_cosine_tile(nseq, ncols, counts, inv_norm, out, kc, blockIdx.x, blockIdx.y, sa, sb);
}
// The cosine matrices of many families in one launch (pgm_kmer_cosine_multi): a block-diagonal grid.  Family f has
// ceil(nseq_f / 16)^2 tiles; tile0[f] is the number of tiles of the families before it (tile0[nfam]: the grid), row0[f] its first
// row in counts and inv_norm, out0[f] the offset of its matrix in out.  A workgroup finds its family by binary search in tile0;
// every element is computed by the code above, so it has the bits pgm_kmer_cosine gives the family alone.
__global__ void __launch_bounds__(PGM_KC_TILE * PGM_KC_TILE) pgm_kmer_cosine_multi_kernel(uint32_t nfam, const uint32_t *__restrict__ tile0, const uint32_t *__restrict__ row0,
                                                                                       const uint64_t *__restrict__ out0, uint32_t ncols, const int32_t *__restrict__ counts,
                                                                                       const double *__restrict__ inv_norm, double *__restrict__ out, uint32_t kc) {
    __shared__ double sa[PGM_KC_TILE][PGM_KC_CHUNK + 1], sb[PGM_KC_TILE][PGM_KC_CHUNK + 1];
    const uint32_t b = blockIdx.x;
    uint32_t lo = 0, hi = nfam;   // the family with tile0[f] <= b < tile0[f + 1] (uniform over the workgroup)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile0[mid] <= b) lo = mid; else hi = mid;
    }
    const uint32_t f = lo, r0 = row0[f], nseq = row0[f + 1] - r0;
    const uint32_t tiles = (nseq + PGM_KC_TILE - 1) / PGM_KC_TILE, t = b - tile0[f];
    pgm_kmer_cosine_tile(nseq, ncols, counts + (size_t)r0 * ncols, inv_norm + r0, out + out0[f], kc, t % tiles, t / tiles, sa, sb);
}
__global__ void pgm_kmer_norm_kernel(uint32_t nseq, uint32_t ncols, const int32_t *__restrict__ counts, double *__restrict__ inv_norm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseq) return;
    unsigned long long ss = 0;
    for (uint32_t k = 0; k < ncols; ++k) { const long long c = counts[(size_t)i * ncols + k]; ss += (unsigned long long)(c * c); }
    inv_norm[i] = __ddiv_rn(1.0, __dsqrt_rn((double)ss));
}

#endif
