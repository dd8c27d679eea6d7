// pgm_agreement_kernels.h — residue-pair agreement between a base alignment and nrep replicate alignments (pgmsa --guidance;
// include/pgm_hip.h: pgm_msa_agreement).  where[r][i][c] (int32, nrep x nrows x ncols) is the column of replicate r that holds
// the residue row i has in base column c, negative for a gap; rows i and j agree in (r, c) when both hold a residue there and
// where[r][i][c] == where[r][j][c].  Two reductions of the same compares, one kernel each:
//
//   pair_hits[i][j] = sum over (r, c)  — pgm_agreement_pairs_kernel: an "equality inner product" over the nrep * ncols axis, tiled
//     like a GEMM.  A workgroup owns one PGM_AGREE_T x PGM_AGREE_T tile of (i, j) on or above the diagonal, every thread a 4 x 4
//     corner of it in registers; the two where slabs of PGM_AGREE_K columns go through LDS, stored column-major so that a thread
//     reads its 4 rows of a column with one 16-byte read.  The (r, c) axis is cut into chunks of PGM_AGREE_K columns of one
//     replicate, and blockIdx.y deals the chunks round robin over gridDim.y workgroups per tile (a few tiles cannot fill the
//     device); every workgroup adds its sums with integer atomics, mirrored below the diagonal.
//   res_hits[i][c] = sum over (r, j != i) — pgm_agreement_residues_kernel: a workgroup owns PGM_AGREE_T rows i x PGM_AGREE_T
//     columns c, every thread one column and 16 of the rows in registers; the rows j pass through LDS PGM_AGREE_T at a time (one
//     4-byte LDS read feeds 16 compares); blockIdx.y deals the replicates round robin.
//
// A gap never agrees: a staged gap becomes -1 on the side of row i and -2 on the side of row j, so the inner loops are a bare
// integer compare.  All sums are integers: the results do not depend on the grid or on the order of the atomics.
#ifndef PGM_AGREEMENT_KERNELS_H_
#define PGM_AGREEMENT_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGM_AGREE_T 64     // rows (and, in the residue kernel, columns) of a workgroup's tile
#define PGM_AGREE_K 32     // columns of one staged chunk of the pair kernel
#define PGM_AGREE_PAD 68   // ints per staged column: 64 rows + 4, keeps 16-byte alignment and spreads the staging stores over the banks

// grid: (tiles on or above the diagonal, nsplit) workgroups of 256; pair_hits zeroed by the caller
__global__ void __launch_bounds__(256) pgm_agreement_pairs_kernel(const int32_t *__restrict__ where, uint32_t nrows, uint32_t ncols, uint32_t nrep,
                                                                  uint32_t ntile, uint32_t *__restrict__ pair_hits) {
    __shared__ __attribute__((aligned(16))) int32_t sA[PGM_AGREE_K][PGM_AGREE_PAD];
    __shared__ __attribute__((aligned(16))) int32_t sB[PGM_AGREE_K][PGM_AGREE_PAD];
    uint32_t ti = 0, rem = blockIdx.x;
    while (rem >= ntile - ti) { rem -= ntile - ti; ++ti; }
    const uint32_t tj = ti + rem;
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = ti * PGM_AGREE_T, j0 = tj * PGM_AGREE_T;
    const uint32_t cchunks = (ncols + PGM_AGREE_K - 1) / PGM_AGREE_K;
    const uint32_t nchunks = nrep * cchunks;   // (nrep * ncols fits 32 bits: checked by the caller)
    uint32_t acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0;

    for (uint32_t q = blockIdx.y; q < nchunks; q += gridDim.y) {
        const uint32_t r = q / cchunks, c0 = (q - r * cchunks) * PGM_AGREE_K;
        const int32_t *rep = where + (size_t)r * nrows * ncols;
#pragma unroll 4
        for (uint32_t e = tid; e < PGM_AGREE_T * PGM_AGREE_K; e += 256) {
            const uint32_t row = e / PGM_AGREE_K, k = e % PGM_AGREE_K, c = c0 + k;
            int32_t va = -1, vb = -2;
            if (c < ncols) {
                if (i0 + row < nrows) { const int32_t v = rep[(size_t)(i0 + row) * ncols + c]; if (v >= 0) va = v; }
                if (j0 + row < nrows) { const int32_t v = rep[(size_t)(j0 + row) * ncols + c]; if (v >= 0) vb = v; }
            }
            sA[k][row] = va;
            sB[k][row] = vb;
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t k = 0; k < PGM_AGREE_K; ++k) {
            const int4 a = *reinterpret_cast<const int4 *>(&sA[k][ty * 4]);
            const int4 b = *reinterpret_cast<const int4 *>(&sB[k][tx * 4]);
            const int32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] += (av[x] == bv[y]) ? 1u : 0u;
        }
        __syncthreads();
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const uint32_t gi = i0 + ty * 4 + (uint32_t)x, gj = j0 + tx * 4 + (uint32_t)y;
            if (gi >= nrows || gj >= nrows || gi == gj || acc[x][y] == 0) continue;
            atomicAdd(&pair_hits[(size_t)gi * nrows + gj], acc[x][y]);
            if (ti != tj) atomicAdd(&pair_hits[(size_t)gj * nrows + gi], acc[x][y]);   // (a diagonal tile holds both orders itself)
        }
}

// grid: (column tiles * row tiles, rsplit) workgroups of 256, blockIdx.x = row tile * ctiles + column tile; res_hits zeroed by the caller
__global__ void __launch_bounds__(256) pgm_agreement_residues_kernel(const int32_t *__restrict__ where, uint32_t nrows, uint32_t ncols, uint32_t nrep,
                                                                     uint32_t ctiles, uint32_t *__restrict__ res_hits) {
    __shared__ int32_t sm[PGM_AGREE_T][PGM_AGREE_T];
    const uint32_t tid = threadIdx.x, cx = tid & 63u, iy = tid >> 6;
    const uint32_t it = blockIdx.x / ctiles, ct = blockIdx.x - it * ctiles;
    const uint32_t c = ct * PGM_AGREE_T + cx, i0 = it * PGM_AGREE_T + iy * 16;
    uint32_t acc[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) acc[m] = 0;

    for (uint32_t r = blockIdx.y; r < nrep; r += gridDim.y) {
        const int32_t *rep = where + (size_t)r * nrows * ncols;
        int32_t v[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            v[m] = -1;
            if (c < ncols && i0 + (uint32_t)m < nrows) { const int32_t w = rep[(size_t)(i0 + (uint32_t)m) * ncols + c]; if (w >= 0) v[m] = w; }
        }
        for (uint32_t j0 = 0; j0 < nrows; j0 += PGM_AGREE_T) {
#pragma unroll
            for (uint32_t e = tid; e < PGM_AGREE_T * PGM_AGREE_T; e += 256) {
                const uint32_t row = e / PGM_AGREE_T, col = e % PGM_AGREE_T, cc = ct * PGM_AGREE_T + col;
                int32_t s = -2;
                if (cc < ncols && j0 + row < nrows) { const int32_t w = rep[(size_t)(j0 + row) * ncols + cc]; if (w >= 0) s = w; }
                sm[row][col] = s;
            }
            __syncthreads();
#pragma unroll 4
            for (uint32_t jj = 0; jj < PGM_AGREE_T; ++jj) {
                const int32_t s = sm[jj][cx];
#pragma unroll
                for (int m = 0; m < 16; ++m) acc[m] += (s == v[m]) ? 1u : 0u;
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) acc[m] -= (v[m] >= 0) ? 1u : 0u;   // (row i met itself among the rows j)
    }
    if (c < ncols) {
#pragma unroll
        for (int m = 0; m < 16; ++m)
            if (i0 + (uint32_t)m < nrows && acc[m] != 0) atomicAdd(&res_hits[(size_t)(i0 + (uint32_t)m) * ncols + c], acc[m]);
    }
}

#endif
