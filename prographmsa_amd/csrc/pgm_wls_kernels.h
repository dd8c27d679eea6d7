// pgm_wls_kernels.h — subtree pair sums of the weighted least-squares guide-tree refinement (reference src/LeastSquares.cpp:
// OptimizeQuartet / OptimizeQuintet aggregate the n x n distance and weight matrices over the 4 or 5 subtrees around an edge).
//
// fp64 contract: every term is the reference's W(k,l) * ((D(k,l) - a_k) - b_l), each operation rounded to nearest
// (__dsub_rn / __dmul_rn / __dadd_rn, and -ffp-contract=off for the rest), added in this fixed order (DESIGN.md "WLS
// refinement"; the host statement is wls_pair_sums_host in host/wls.cpp):
//   1. row k of subtree p (one wavefront): lane t adds the terms of the columns l = t, t + 64, ... (ascending) whose subtree q
//      is above p, one accumulator per q; the 64 lanes are combined by the xor butterfly 32, 16, 8, 4, 2, 1 (v += v^m)
//   2. a workgroup holds PGM_WLS_ROWS consecutive rows; wave v takes the rows v, v + 4, v + 8, v + 12 of them and adds each
//      row's sums, in that order, into its pair slots; the block's partial is (wave0 + wave1) + (wave2 + wave3)
//   3. per job, lane t adds the partials of the blocks t, t + 64, ... (ascending) and the lanes are combined as in 1.
// The results do not depend on the number of jobs in a call or on the device.
#ifndef PGM_WLS_KERNELS_H_
#define PGM_WLS_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGM_WLS_ROWS 16    // rows per workgroup of the first kernel (4 wavefronts x 4 rows)
#define PGM_WLS_SLOTS 20   // per job: 10 pair sums, then 10 weight sums (PGM_WLS_OUT)

struct PgmWlsJobDev {
    const int8_t *label;
    const double *offset;
    uint32_t nsub;
};

__device__ __forceinline__ double pgm_wls_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = __dadd_rn(v, __shfl_xor(v, m, 64));
    return v;
}

// first pair slot of subtree p (pairs (p, q > p) in lexicographic order)
__device__ __forceinline__ int pgm_wls_base(int p, int K) { return p * K - p * (p + 1) / 2; }

// grid: nblocks x njobs workgroups of 256 (block b of job j = blockIdx.x j * nblocks + b); dw: (D, W) pairs, row-major n x n;
// part: per (job, block) PGM_WLS_SLOTS partial sums
__global__ void __launch_bounds__(256) pgm_wls_rows_kernel(const double2 *__restrict__ dw, uint32_t n, const PgmWlsJobDev *__restrict__ jobs,
                                                           uint32_t nblocks, double *__restrict__ part) {
    const uint32_t job = blockIdx.x / nblocks, blk = blockIdx.x % nblocks;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const PgmWlsJobDev J = jobs[job];
    const int K = (int)J.nsub;
    double acc[PGM_WLS_SLOTS];
#pragma unroll
    for (int s = 0; s < PGM_WLS_SLOTS; ++s) acc[s] = 0.0;
    for (uint32_t i = 0; i < PGM_WLS_ROWS / 4; ++i) {
        const uint32_t k = blk * PGM_WLS_ROWS + wave + 4u * i;
        if (k >= n) break;
        const int p = J.label[k];
        if (p < 0 || p >= K - 1) continue;   // (wave-uniform) no subtree above p: nothing to add
        const double a = J.offset[k];
        const double2 *row = dw + (size_t)k * n;
        double s[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (uint32_t l = lane; l < n; l += 64u) {
            const int j = (int)J.label[l] - p - 1;   // accumulator of subtree q = p + 1 + j (j < 0: not above p)
            const double2 e = row[l];
            const double term = __dmul_rn(e.y, __dsub_rn(__dsub_rn(e.x, a), J.offset[l]));
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (j == jj) { s[jj] = __dadd_rn(s[jj], term); w[jj] = __dadd_rn(w[jj], e.y); }
        }
        const int base = pgm_wls_base(p, K), cnt = K - 1 - p;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const double rs = pgm_wls_wave_sum(s[jj]), rw = pgm_wls_wave_sum(w[jj]);
#pragma unroll
            for (int q = 0; q < 10; ++q)
                if (jj < cnt && q == base + jj) { acc[q] = __dadd_rn(acc[q], rs); acc[10 + q] = __dadd_rn(acc[10 + q], rw); }
        }
    }
    __shared__ double red[4][PGM_WLS_SLOTS];
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < PGM_WLS_SLOTS; ++q) red[wave][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < PGM_WLS_SLOTS) {
        const int q = threadIdx.x;
        part[(size_t)blockIdx.x * PGM_WLS_SLOTS + q] = __dadd_rn(__dadd_rn(red[0][q], red[1][q]), __dadd_rn(red[2][q], red[3][q]));
    }
}

// one wavefront per job: the job's nblocks partials -> out[PGM_WLS_SLOTS * job ..]
__global__ void __launch_bounds__(64) pgm_wls_jobs_kernel(const double *__restrict__ part, uint32_t nblocks, double *__restrict__ out) {
    const uint32_t job = blockIdx.x, lane = threadIdx.x;
    double acc[PGM_WLS_SLOTS];
#pragma unroll
    for (int q = 0; q < PGM_WLS_SLOTS; ++q) acc[q] = 0.0;
    for (uint32_t b = lane; b < nblocks; b += 64u) {
        const double *src = part + ((size_t)job * nblocks + b) * PGM_WLS_SLOTS;
#pragma unroll
        for (int q = 0; q < PGM_WLS_SLOTS; ++q) acc[q] = __dadd_rn(acc[q], src[q]);
    }
#pragma unroll
    for (int q = 0; q < PGM_WLS_SLOTS; ++q) {
        const double v = pgm_wls_wave_sum(acc[q]);
        if (lane == 0) out[(size_t)job * PGM_WLS_SLOTS + q] = v;
    }
}

#endif
