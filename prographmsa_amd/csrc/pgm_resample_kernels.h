// pgm_resample_kernels.h — sums of the rows of a matrix over resampled columns (pgmsa --ml_tree --ml_support; include/pgm_hip.h:
// pgm_resampled_sums):
//
//   out[q][r] = x[q][cols[r][0]] + x[q][cols[r][1]] + ... , k ascending, from 0.0, every step one fp64 addition
//
// x arrives [q][s]; lanes over q would read it at a stride of 8 ncols bytes.  pgm_resample_transpose_kernel writes it once as
// xt[s][q], 32 x 32 tiles through LDS, the row pitch a multiple of PGM_RESAMPLE_T with the rows beyond nrow zero, so that the sums'
// kernel reads without a bound.
//
// pgm_resample_sums_kernel: a wavefront owns PGM_RESAMPLE_T = 64 rows q (one a lane) and PGM_RESAMPLE_R = 4 replicates; a thread
// carries the four sums of its row as independent add chains.  cols[r][k] is the same for the whole wavefront: it is read through
// wave-uniform pointers (scalar loads, once a wavefront), and the gather of step k is one coalesced 512-byte read of row cols[r][k]
// of xt per replicate.  A workgroup is four wavefronts on one q-tile: 16 replicates.  Every workgroup of a q-tile re-reads the same
// ncols x 64 slice of xt, so the items are numbered for them to meet in one XCD's L2: workgroups go to the 8 XCDs round robin by
// their index, item i belongs to XCD i % 8, and the items of an XCD walk one q-tile's replicate groups before the next q-tile's.
// The grid is one dimension with a uniform stride loop (a multiple of 8 workgroups, so an item keeps its XCD).  One writer per out
// entry, no atomics, nothing zeroed, no workgroup waits for another; the order of the additions is the statement's whatever the launch.
#ifndef PGM_RESAMPLE_KERNELS_H_
#define PGM_RESAMPLE_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGM_RESAMPLE_T 64        // rows of a q-tile: one a lane
#define PGM_RESAMPLE_R 4         // replicates a thread carries
#define PGM_RESAMPLE_WAVES 4     // wavefronts of a workgroup
#define PGM_RESAMPLE_GROUP (PGM_RESAMPLE_R * PGM_RESAMPLE_WAVES)   // replicates of a workgroup
#define PGM_RESAMPLE_XCDS 8
#define PGM_RESAMPLE_MAXGRID 2048u   // workgroups of the sums' kernel at the most (a multiple of PGM_RESAMPLE_XCDS); items beyond are strided over

// grid: (ceil(ncols / 32), min(pitch / 32, 65535)) workgroups of 256; pitch % 64 == 0
__global__ __launch_bounds__(256) void pgm_resample_transpose_kernel(const double *__restrict__ x, uint32_t nrow, uint32_t ncols, size_t pitch, double *__restrict__ xt) {
    __shared__ double tile[32][33];
    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5, s0 = blockIdx.x * 32u, qtiles = (uint32_t)(pitch / 32u);
    for (uint32_t by = blockIdx.y; by < qtiles; by += gridDim.y) {   // (uniform over the workgroup)
        const size_t q0 = (size_t)by * 32u;
#pragma unroll
        for (uint32_t j = 0; j < 32; j += 8) {
            const size_t q = q0 + ty + j;
            const uint32_t s = s0 + tx;
            tile[ty + j][tx] = q < nrow && s < ncols ? x[q * ncols + s] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < 32; j += 8) {
            const uint32_t s = s0 + ty + j;
            if (s < ncols) xt[(size_t)s * pitch + q0 + tx] = tile[tx][ty + j];
        }
        __syncthreads();
    }
}

// grid: min(nitems, PGM_RESAMPLE_MAXGRID) workgroups of 64 * PGM_RESAMPLE_WAVES; nitems = 8 * ceil(qtiles / 8) * ngroups, qtiles = pitch / 64,
// ngroups = ceil(nrep / PGM_RESAMPLE_GROUP); every cols entry < ncols (the entry checks it)
__global__ __launch_bounds__(64 * PGM_RESAMPLE_WAVES) void pgm_resample_sums_kernel(const double *__restrict__ xt, uint32_t nrow, uint32_t ncols, size_t pitch,
                                                                                    uint32_t nrep, const uint32_t *__restrict__ cols, uint64_t nitems, uint32_t ngroups,
                                                                                    double *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t qtiles = pitch / PGM_RESAMPLE_T;
    for (uint64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const uint64_t j = item / PGM_RESAMPLE_XCDS;
        const uint64_t tile = j / ngroups * PGM_RESAMPLE_XCDS + item % PGM_RESAMPLE_XCDS;
        const uint32_t r0 = (uint32_t)(j % ngroups) * PGM_RESAMPLE_GROUP + wave * PGM_RESAMPLE_R;
        if (tile >= qtiles || r0 >= nrep) continue;   // (the padding of the last round of XCDs; a wavefront beyond the replicates)
        const size_t q = (size_t)tile * PGM_RESAMPLE_T + lane;
        const uint32_t last = nrep - 1;
        // a replicate beyond the last repeats the last and is not written
        const uint32_t *c0 = cols + (size_t)r0 * ncols, *c1 = cols + (size_t)min(r0 + 1, last) * ncols;
        const uint32_t *c2 = cols + (size_t)min(r0 + 2, last) * ncols, *c3 = cols + (size_t)min(r0 + 3, last) * ncols;
        const double *col = xt + q;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
        for (uint32_t k = 0; k < ncols; ++k) {
            const double v0 = col[(size_t)c0[k] * pitch], v1 = col[(size_t)c1[k] * pitch], v2 = col[(size_t)c2[k] * pitch], v3 = col[(size_t)c3[k] * pitch];
            a0 = a0 + v0; a1 = a1 + v1; a2 = a2 + v2; a3 = a3 + v3;
        }
        if (q < nrow) {
            double *o = out + q * nrep + r0;
            o[0] = a0;
            if (r0 + 1 < nrep) o[1] = a1;
            if (r0 + 2 < nrep) o[2] = a2;
            if (r0 + 3 < nrep) o[3] = a3;
        }
    }
}

#endif
