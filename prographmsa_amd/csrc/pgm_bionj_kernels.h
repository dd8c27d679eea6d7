// pgm_bionj_kernels.h — the joins of BioNJ (reference src/TreeNJ.cpp:132-281; the host statement is bionj_joins_host in
// host/bionj.cpp) for many families at once, three kernels per join, the families lock-stepped over the join number.
//
// fp64 contract: every value is the host's expression, operation by operation (IEEE add, sub, mul, div and strict comparisons;
// the library is built with -ffp-contract=off -fno-fast-math), and every order-sensitive sum is the host's order:
//   * a column sum is eigen_column_sum over the reduced index order: start = (j dim) & 1, four accumulators over the elements
//     start + 4 t + {0, 1, 2, 3}, a0 += b0, a1 += b1, an odd last pair added to (a0, a1), a0 + a1, then the head element and
//     the tail element.  The four accumulators are four lanes of the column's wavefront; the others stage the column in LDS.
//   * the criterion's winner is the first strict minimum in column-major order (row fastest): candidates are ordered by
//     (q, col dim + row) with == on q for the tie
//   * vsum is one lane's sequential sum over i ascending of the differences staged in LDS
// The matrices stay in their n x n storage; `act` lists the rows / columns still in the reduced matrix (ping-pong: join s reads
// act[s & 1] and writes act[(s + 1) & 1]).  T is the transpose of D (the sums and the criterion read columns).  The entries a
// join writes are clamped when they are written (the host clamps them at the start of the next join and nothing reads them in
// between), except by a family's last join: the host clamps nothing after it.
// Stream order is the only dependency between the kernels: no grid-wide barrier, no flag.
#ifndef PGM_BIONJ_KERNELS_H_
#define PGM_BIONJ_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/pgm_hip.h"

#define PGM_BIONJ_MIN_DIST 1e-4
#define PGM_BIONJ_MIN_VAR 1e-5
#define PGM_BIONJ_CHUNK 1024   // elements of a column (of the vsum differences) staged in LDS at a time
#define PGM_BIONJ_COLS 4       // columns per workgroup of the sums and scan kernels (one wavefront each)

struct PgmBionjFam {
    uint32_t n;
    uint64_t moff;   // first element of the family's matrices in D, T, V
    uint64_t voff;   // first element of its vectors: act (2 x), sums, best_q, best_row
    uint64_t joff;   // first record of its join log
};
struct PgmBionjDev {
    const PgmBionjFam *fam;
    uint32_t nfam;
    double *D, *T, *V;
    uint32_t *act[2];
    double *sums, *best_q;
    uint32_t *best_row;
    pgm_bionj_join *joins;
    double *final_d;
};

__device__ __forceinline__ double pgm_bionj_max(double a, double b) { return a < b ? b : a; }   // std::max(a, b)
__device__ __forceinline__ double pgm_bionj_min(double a, double b) { return b < a ? b : a; }   // std::min(a, b)
__device__ __forceinline__ uint32_t pgm_bionj_family(void) { return blockIdx.y + blockIdx.z * gridDim.y; }

// Column sums of join `step`.  grid: (columns / PGM_BIONJ_COLS, families), 64 PGM_BIONJ_COLS threads; wavefront w of a block
// sums column blockIdx.x PGM_BIONJ_COLS + w.  At step 0 the wavefront of column j first clamps column j of D (writing T with
// it) and row j of V and zeroes their diagonal elements: together the host's clamp of the whole matrix.
__global__ void __launch_bounds__(64 * PGM_BIONJ_COLS) pgm_bionj_sums_kernel(PgmBionjDev S, uint32_t step) {
    __shared__ double stage[PGM_BIONJ_COLS][PGM_BIONJ_CHUNK];
    const uint32_t f = pgm_bionj_family();
    if (f >= S.nfam) return;
    const PgmBionjFam F = S.fam[f];
    if (F.n < step + 4u) return;   // three clusters left
    const uint32_t n = F.n, dim = n - step, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (blockIdx.x * PGM_BIONJ_COLS >= dim) return;   // (block-uniform)
    const uint32_t jw = blockIdx.x * PGM_BIONJ_COLS + wave;
    const bool on = jw < dim;   // (a wavefront past the last column keeps the block's barriers company)
    const uint32_t j = on ? jw : 0u;
    const uint32_t *act = S.act[step & 1u] + F.voff;
    const uint32_t aj = act[j];
    double *D = S.D + F.moff, *V = S.V + F.moff;
    double *col = S.T + F.moff + (size_t)aj * n;
    const uint32_t start = (uint32_t)(((uint64_t)j * dim) & 1u);
    const uint32_t end2 = start + ((dim - start) / 4u) * 4u, end = start + ((dim - start) / 2u) * 2u;   // (dim >= 4: end2 > start)
    double *st = stage[wave];
    double acc = 0.0, head = 0.0, odd = 0.0, tail = 0.0;   // lane q < 4: accumulator q; lanes 0, 1: the odd last pair
    for (uint32_t k0 = 0; k0 < dim; k0 += PGM_BIONJ_CHUNK) {
        const uint32_t kn = min((uint32_t)PGM_BIONJ_CHUNK, dim - k0);
        if (on && step == 0u) {   // (act is the identity: i is a row of the matrix)
            for (uint32_t i = k0 + lane; i < k0 + kn; i += 64u) {
                const double d = i == j ? 0.0 : pgm_bionj_max(D[(size_t)i * n + j], PGM_BIONJ_MIN_DIST);
                D[(size_t)i * n + j] = d;
                col[i] = d;
                V[(size_t)j * n + i] = i == j ? 0.0 : pgm_bionj_max(V[(size_t)j * n + i], PGM_BIONJ_MIN_VAR);
                st[i - k0] = d;
            }
        } else if (on) {
            for (uint32_t k = lane; k < kn; k += 64u) st[k] = col[act[k0 + k]];
        }
        __syncthreads();
        if (on && lane < 4u) {
            // the elements start + 4 t + lane inside [k0, k0 + kn) and below end2, ascending; the first one starts the accumulator
            uint32_t k = start + lane;
            if (k < k0) k += (k0 - k + 3u) / 4u * 4u;
            const uint32_t stop = min(end2, k0 + kn);
            if (k == start + lane && k < stop) { acc = st[k - k0]; k += 4u; }
            for (; k < stop; k += 4u) acc += st[k - k0];
            if (lane < 2u && end > end2 && end2 + lane >= k0 && end2 + lane < k0 + kn) odd = st[end2 + lane - k0];
            if (lane == 0u) {
                if (k0 == 0u && start) head = st[0];
                if (end < dim && dim - 1u >= k0 && dim - 1u < k0 + kn) tail = st[dim - 1u - k0];
            }
        }
        __syncthreads();
    }
    if (!on) return;
    // a0 += b0; a1 += b1 (lanes 0, 1 take the accumulators of lanes 2, 3); the odd pair; a0 + a1; head; tail
    const double other = __shfl(acc, (int)(lane + 2u) & 63, 64);
    if (lane < 2u) {
        acc += other;
        if (end > end2) acc += odd;
    }
    const double a1 = __shfl(acc, 1, 64);
    if (lane == 0u) {
        double res = acc + a1;
        if (start) res += head;
        if (end < dim) res += tail;
        S.sums[F.voff + j] = res;
    }
}

// The criterion of join `step`: per column the first minimum over the rows.  grid and block as for the sums.
__global__ void __launch_bounds__(64 * PGM_BIONJ_COLS) pgm_bionj_scan_kernel(PgmBionjDev S, uint32_t step) {
    const uint32_t f = pgm_bionj_family();
    if (f >= S.nfam) return;
    const PgmBionjFam F = S.fam[f];
    if (F.n < step + 4u) return;
    const uint32_t n = F.n, dim = n - step, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t colj = blockIdx.x * PGM_BIONJ_COLS + wave;
    if (colj >= dim) return;
    const uint32_t *act = S.act[step & 1u] + F.voff;
    const double *sums = S.sums + F.voff;
    const double *colp = S.T + F.moff + (size_t)act[colj] * n;
    const double fq = 0.5 / ((double)(int)dim - 2.0);
    const double sc = sums[colj];
    double bq = INFINITY;
    uint32_t brow = 0xFFFFFFFFu;
    for (uint32_t row = lane; row < dim; row += 64u) {   // (ascending per lane: the strict comparison keeps the lane's first)
        if (row == colj) continue;
        const double q = 0.5 * colp[act[row]] - fq * (sc + sums[row]);
        if (q < bq) { bq = q; brow = row; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oq = __shfl_xor(bq, m, 64);
        const uint32_t orow = __shfl_xor(brow, m, 64);
        if (oq < bq || (oq == bq && orow < brow)) { bq = oq; brow = orow; }
    }
    if (lane == 0u) { S.best_q[F.voff + colj] = bq; S.best_row[F.voff + colj] = brow; }
}

// The join of step `step`: one workgroup of 256 per family.  The winner over the columns, dist1, dist2, vsum, lambda, the new
// row / column index1 of D, T and V, the reduced index list without index2, the join record; the family's last join also
// writes final_d.
__global__ void __launch_bounds__(256) pgm_bionj_join_kernel(PgmBionjDev S, uint32_t step) {
    __shared__ double sq[256];
    __shared__ uint32_t scol[256], srow[256];
    __shared__ double diff[PGM_BIONJ_CHUNK];
    __shared__ double s_vsum, s_nd4[4];
    const uint32_t f = pgm_bionj_family();
    if (f >= S.nfam) return;
    const PgmBionjFam F = S.fam[f];
    if (F.n < step + 4u) return;
    const uint32_t n = F.n, dim = n - step, tid = threadIdx.x;
    const uint32_t *act = S.act[step & 1u] + F.voff;
    uint32_t *act_next = S.act[(step + 1u) & 1u] + F.voff;
    const double *sums = S.sums + F.voff;
    double *D = S.D + F.moff, *T = S.T + F.moff, *V = S.V + F.moff;
    // ---- the first minimum in column-major order: (q, col) ascending over the columns' own first minima
    double bq = INFINITY;
    uint32_t bcol = 0xFFFFFFFFu, brow = 0xFFFFFFFFu;
    for (uint32_t c = tid; c < dim; c += 256u) {
        const double q = S.best_q[F.voff + c];
        if (q < bq) { bq = q; bcol = c; brow = S.best_row[F.voff + c]; }
    }
    sq[tid] = bq; scol[tid] = bcol; srow[tid] = brow;
    __syncthreads();
    for (uint32_t m = 128u; m >= 1u; m >>= 1) {
        if (tid < m) {
            const double oq = sq[tid + m];
            const uint32_t oc = scol[tid + m];
            if (oq < sq[tid] || (oq == sq[tid] && oc < scol[tid])) { sq[tid] = oq; scol[tid] = oc; srow[tid] = srow[tid + m]; }
        }
        __syncthreads();
    }
    uint32_t index1 = 0, index2 = 0;   // (the host's scan starts from +inf at (0, 0) and takes strictly smaller values only)
    if (sq[0] < INFINITY) { index2 = srow[0]; index1 = scol[0]; }
    if (index2 < index1) { const uint32_t t = index1; index1 = index2; index2 = t; }
    const uint32_t a1 = act[index1], a2 = act[index2];
    const double *D1 = D + (size_t)a1 * n, *D2 = D + (size_t)a2 * n, *V1 = V + (size_t)a1 * n, *V2 = V + (size_t)a2 * n;
    const double ddim2 = (double)(int)dim - 2.0;
    const double d12 = D1[a2];
    double dist1 = (d12 + (sums[index1] - sums[index2]) / ddim2) / 2.0;
    dist1 = pgm_bionj_min(pgm_bionj_max(dist1, PGM_BIONJ_MIN_DIST), d12);
    const double dist2 = pgm_bionj_max(D2[a1] - dist1, PGM_BIONJ_MIN_DIST);
    // ---- vsum: the differences through LDS, thread 0 adds them in order
    double vsum = 0;
    for (uint32_t k0 = 0; k0 < dim; k0 += PGM_BIONJ_CHUNK) {
        const uint32_t kn = min((uint32_t)PGM_BIONJ_CHUNK, dim - k0);
        for (uint32_t k = tid; k < kn; k += 256u) { const uint32_t ai = act[k0 + k]; diff[k] = V2[ai] - V1[ai]; }
        __syncthreads();
        if (tid == 0u)
            for (uint32_t k = 0; k < kn; ++k) vsum += diff[k];
        __syncthreads();
    }
    if (tid == 0u) s_vsum = vsum;
    __syncthreads();
    vsum = s_vsum;
    const double v12 = V1[a2];
    double lambda = .5 + vsum / ((double)(2 * ((int)dim - 2)) * v12);
    if (isnan(lambda)) lambda = .5;
    else lambda = pgm_bionj_min(pgm_bionj_max(0.0, lambda), 1.0);
    // ---- the joined cluster in row / column index1; thread i reads and writes the entries of reduced index i only, and no
    // entry of (index1, index2) or (index2, index1) is written
    const bool last = dim == 4u;
    for (uint32_t i = tid; i < dim; i += 256u) {
        if (i == index2) continue;
        const uint32_t ai = act[i];
        double nd = lambda * (D1[ai] - dist1) + (1.0 - lambda) * (D2[ai] - dist2);
        double nv = lambda * V1[ai] + (1.0 - lambda) * V2[ai] - lambda * (1.0 - lambda) * v12;
        if (i == index1) { nd = 0; nv = 0; }
        else if (!last) { nd = pgm_bionj_max(nd, PGM_BIONJ_MIN_DIST); nv = pgm_bionj_max(nv, PGM_BIONJ_MIN_VAR); }
        if (last) s_nd4[i] = nd;
        D[(size_t)a1 * n + ai] = nd; D[(size_t)ai * n + a1] = nd;
        T[(size_t)a1 * n + ai] = nd; T[(size_t)ai * n + a1] = nd;
        V[(size_t)a1 * n + ai] = nv; V[(size_t)ai * n + a1] = nv;
    }
    for (uint32_t i = tid; i + 1u < dim; i += 256u) act_next[i] = act[i < index2 ? i : i + 1u];
    if (tid == 0u) {
        pgm_bionj_join r;
        r.index1 = index1; r.index2 = index2; r.dist1 = dist1; r.dist2 = dist2;
        S.joins[F.joff + step] = r;
    }
    if (last) {   // (block-uniform) D of the three clusters left: the entries of index1 as just computed, the others as stored
        __syncthreads();
        if (tid < 9u) {
            const uint32_t r = tid / 3u, c = tid % 3u;
            const uint32_t orow = r < index2 ? r : r + 1u, ocol = c < index2 ? c : c + 1u;   // reduced indices before the join
            double v;
            if (orow == index1) v = s_nd4[ocol];
            else if (ocol == index1) v = s_nd4[orow];
            else v = D[(size_t)act[orow] * n + act[ocol]];
            S.final_d[(size_t)9 * f + tid] = v;
        }
    }
}

// ---- the joins of a fixed topology (pgm_bionj_plan_multi; the host statement is bionj_joins_host with a plan) ------------------
// The pair of every join is given, so a join needs the column sums of its two columns only and no criterion: O(dim) work, and
// nothing but the matrix carries over from one join to the next.  One launch clamps the matrices, one more runs every join: a
// workgroup per family loops over the family's joins.  The fp64 contract is the one above: the two sums in eigen_column_sum's
// association (wavefronts 0 and 1: the column staged in LDS, lanes 0-3 the four accumulators), vsum one lane's sum in index
// order (wavefront 2), dist1, dist2 and lambda the host's expressions on one lane, the new row / column clamped as it is
// written except by the last join.
// A workgroup reads global memory that the preparation launch or the workgroup itself wrote, never another workgroup's, so
// __syncthreads() (the barrier and its workgroup-scope fence) between a phase's stores and the next phase's loads is all the
// synchronisation there is: no flag, nothing spins, no workgroup waits for another.

// The host's clamp of the whole matrix before the first join, and T.  grid: (blocks, families), grid-stride over the elements.
__global__ void __launch_bounds__(256) pgm_bionj_prepare_kernel(PgmBionjDev S) {
    const uint32_t f = pgm_bionj_family();
    if (f >= S.nfam) return;
    const PgmBionjFam F = S.fam[f];
    const uint64_t n = F.n, nn = n * n;
    double *D = S.D + F.moff, *T = S.T + F.moff, *V = S.V + F.moff;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < nn; e += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = e / n, j = e - i * n;
        const double d = i == j ? 0.0 : pgm_bionj_max(D[e], PGM_BIONJ_MIN_DIST);
        D[e] = d;
        T[j * n + i] = d;
        V[e] = i == j ? 0.0 : pgm_bionj_max(V[e], PGM_BIONJ_MIN_VAR);
    }
}

// All joins of a family: one workgroup of 256 per family, grid (1, families).  plan holds the pairs as S.joins holds the records
// (family f: from F.joff on).
__global__ void __launch_bounds__(256) pgm_bionj_plan_kernel(PgmBionjDev S, const pgm_bionj_pair *plan) {
    __shared__ double stage[2][PGM_BIONJ_CHUNK];   // the columns of index1 and index2
    __shared__ double diff[PGM_BIONJ_CHUNK];       // V(index2, i) - V(index1, i)
    __shared__ double s_sum[2], s_vsum, s_par[3], s_nd4[4];
    const uint32_t f = pgm_bionj_family();
    if (f >= S.nfam) return;
    const PgmBionjFam F = S.fam[f];
    const uint32_t n = F.n, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    double *D = S.D + F.moff, *T = S.T + F.moff, *V = S.V + F.moff;
    for (uint32_t step = 0; step + 3u < n; ++step) {   // (every bound of the loops below is the same for the whole workgroup)
        const uint32_t dim = n - step;
        const uint32_t *act = S.act[step & 1u] + F.voff;
        uint32_t *act_next = S.act[(step + 1u) & 1u] + F.voff;
        const uint32_t index1 = plan[F.joff + step].index1, index2 = plan[F.joff + step].index2;
        const uint32_t a1 = act[index1], a2 = act[index2];
        const double *D1 = D + (size_t)a1 * n, *D2 = D + (size_t)a2 * n, *V1 = V + (size_t)a1 * n, *V2 = V + (size_t)a2 * n;
        // ---- the two column sums and vsum
        const uint32_t j = wave == 0u ? index1 : index2;   // (wavefronts 0 and 1)
        const double *col = T + (size_t)(wave == 0u ? a1 : a2) * n;   // column j of D
        const uint32_t start = (uint32_t)(((uint64_t)j * dim) & 1u);
        const uint32_t end2 = start + ((dim - start) / 4u) * 4u, end = start + ((dim - start) / 2u) * 2u;   // (dim >= 4: end2 > start)
        double acc = 0.0, head = 0.0, odd = 0.0, tail = 0.0, vsum = 0.0;
        for (uint32_t k0 = 0; k0 < dim; k0 += PGM_BIONJ_CHUNK) {
            const uint32_t kn = min((uint32_t)PGM_BIONJ_CHUNK, dim - k0);
            if (wave < 2u) {
                double *st = stage[wave];
                for (uint32_t k = lane; k < kn; k += 64u) st[k] = col[act[k0 + k]];
            } else if (wave == 2u) {
                for (uint32_t k = lane; k < kn; k += 64u) { const uint32_t ai = act[k0 + k]; diff[k] = V2[ai] - V1[ai]; }
            }
            __syncthreads();
            if (wave < 2u && lane < 4u) {
                // the elements start + 4 t + lane inside [k0, k0 + kn) and below end2, ascending; the first one starts the accumulator
                const double *st = stage[wave];
                uint32_t k = start + lane;
                if (k < k0) k += (k0 - k + 3u) / 4u * 4u;
                const uint32_t stop = min(end2, k0 + kn);
                if (k == start + lane && k < stop) { acc = st[k - k0]; k += 4u; }
                for (; k < stop; k += 4u) acc += st[k - k0];
                if (lane < 2u && end > end2 && end2 + lane >= k0 && end2 + lane < k0 + kn) odd = st[end2 + lane - k0];
                if (lane == 0u) {
                    if (k0 == 0u && start) head = st[0];
                    if (end < dim && dim - 1u >= k0 && dim - 1u < k0 + kn) tail = st[dim - 1u - k0];
                }
            } else if (tid == 128u) {
                for (uint32_t k = 0; k < kn; ++k) vsum += diff[k];
            }
            __syncthreads();
        }
        if (wave < 2u) {   // a0 += b0; a1 += b1 (lanes 0, 1 take the accumulators of lanes 2, 3); the odd pair; a0 + a1; head; tail
            const double other = __shfl(acc, (int)(lane + 2u) & 63, 64);
            if (lane < 2u) {
                acc += other;
                if (end > end2) acc += odd;
            }
            const double acc1 = __shfl(acc, 1, 64);
            if (lane == 0u) {
                double res = acc + acc1;
                if (start) res += head;
                if (end < dim) res += tail;
                s_sum[wave] = res;
            }
        } else if (tid == 128u) {
            s_vsum = vsum;
        }
        __syncthreads();
        // ---- dist1, dist2, lambda: the host's expressions on one lane
        if (tid == 0u) {
            const double ddim2 = (double)(int)dim - 2.0;
            const double d12 = D1[a2];
            double dist1 = (d12 + (s_sum[0] - s_sum[1]) / ddim2) / 2.0;
            dist1 = pgm_bionj_min(pgm_bionj_max(dist1, PGM_BIONJ_MIN_DIST), d12);
            const double dist2 = pgm_bionj_max(D2[a1] - dist1, PGM_BIONJ_MIN_DIST);
            double lambda = .5 + s_vsum / ((double)(2 * ((int)dim - 2)) * V1[a2]);
            if (isnan(lambda)) lambda = .5;
            else lambda = pgm_bionj_min(pgm_bionj_max(0.0, lambda), 1.0);
            s_par[0] = dist1; s_par[1] = dist2; s_par[2] = lambda;
            pgm_bionj_join r;
            r.index1 = index1; r.index2 = index2; r.dist1 = dist1; r.dist2 = dist2;
            S.joins[F.joff + step] = r;
        }
        __syncthreads();
        const double dist1 = s_par[0], dist2 = s_par[1], lambda = s_par[2];
        const double v12 = V1[a2];
        // ---- the joined cluster in row / column index1; thread i reads and writes the entries of reduced index i only, and no
        // entry of (index1, index2) or (index2, index1) is written
        const bool last = dim == 4u;
        for (uint32_t i = tid; i < dim; i += 256u) {
            if (i == index2) continue;
            const uint32_t ai = act[i];
            double nd = lambda * (D1[ai] - dist1) + (1.0 - lambda) * (D2[ai] - dist2);
            double nv = lambda * V1[ai] + (1.0 - lambda) * V2[ai] - lambda * (1.0 - lambda) * v12;
            if (i == index1) { nd = 0; nv = 0; }
            else if (!last) { nd = pgm_bionj_max(nd, PGM_BIONJ_MIN_DIST); nv = pgm_bionj_max(nv, PGM_BIONJ_MIN_VAR); }
            if (last) s_nd4[i] = nd;
            D[(size_t)a1 * n + ai] = nd; D[(size_t)ai * n + a1] = nd;
            T[(size_t)a1 * n + ai] = nd; T[(size_t)ai * n + a1] = nd;
            V[(size_t)a1 * n + ai] = nv; V[(size_t)ai * n + a1] = nv;
        }
        for (uint32_t i = tid; i + 1u < dim; i += 256u) act_next[i] = act[i < index2 ? i : i + 1u];
        __syncthreads();   // (the next join reads what this one wrote)
        if (last && tid < 9u) {   // D of the three clusters left: the entries of index1 as just computed, the others as stored
            const uint32_t r = tid / 3u, c = tid % 3u;
            const uint32_t orow = r < index2 ? r : r + 1u, ocol = c < index2 ? c : c + 1u;   // reduced indices before the join
            double v;
            if (orow == index1) v = s_nd4[ocol];
            else if (ocol == index1) v = s_nd4[orow];
            else v = D[(size_t)act[orow] * n + act[ocol]];
            S.final_d[(size_t)9 * f + tid] = v;
        }
    }
}

#endif
