// pgm_transfer_kernels.h — transfer indices of the bipartitions of a reference tree against the bipartitions of nrep replicate
// trees (pgmsa --bootstrap_tbe; include/pgm_hip.h: pgm_transfer_min).  A bipartition is a bit set over nleaves leaves; with
// h = popcount(A xor B), the transfer distance of two sets is min(h, nleaves - h), and
//
//   phi[e][r] = min(p(A_e) - 1, min over the sets B of replicate r of the distance of A_e and B)
//
// pgm_transfer_min_kernel: a "Hamming inner product" with a minimum for the reduction, tiled like pgm_agreement_pairs_kernel.  The
// sets are read as 32-bit words (two to a uint64, little endian).  A workgroup owns PGM_TRANSFER_T reference sets and walks the sets
// of a replicate PGM_TRANSFER_T at a time, every thread a 4 x 4 corner of Hamming sums in registers; the two slabs of
// PGM_TRANSFER_K words go through LDS, stored word-major so that a thread reads its 4 sets of a word with one 16-byte read.  When
// the words of a tile are through, min(h, nleaves - h) of the columns that exist is folded into a running minimum per reference
// row; at the end of the replicate the 16 threads that share a row reduce it across lanes and one of them writes phi.  blockIdx.y
// deals the replicates round robin.  Every phi entry has one writer: no atomics, nothing zeroed, no workgroup waits for another.
#ifndef PGM_TRANSFER_KERNELS_H_
#define PGM_TRANSFER_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGM_TRANSFER_T 64     // sets of a tile, on either side
#define PGM_TRANSFER_K 32     // 32-bit words of one staged chunk
#define PGM_TRANSFER_PAD 68   // words per staged row: 64 sets + 4, keeps 16-byte alignment and spreads the staging stores over the banks

// grid: (tiles of PGM_TRANSFER_T reference sets, replicate lanes) workgroups of 256; words32 = 2 * ((nleaves + 63) / 64)
__global__ void __launch_bounds__(256) pgm_transfer_min_kernel(const uint32_t *__restrict__ ref, uint32_t nref, const uint32_t *__restrict__ rep,
                                                               const uint32_t *__restrict__ rep_off, uint32_t nrep, uint32_t nleaves, uint32_t words32,
                                                               uint32_t *__restrict__ phi) {
    __shared__ __attribute__((aligned(16))) uint32_t sA[PGM_TRANSFER_K][PGM_TRANSFER_PAD];
    __shared__ __attribute__((aligned(16))) uint32_t sB[PGM_TRANSFER_K][PGM_TRANSFER_PAD];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = blockIdx.x * PGM_TRANSFER_T, nrow = min((uint32_t)PGM_TRANSFER_T, nref - i0);   // (i0 < nref: the grid has no empty tile)

    // p - 1 of the thread's four reference rows, from the sets themselves: the 16 threads of a row share its words
    uint32_t clamp[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const uint32_t row = ty * 4 + (uint32_t)x;
        uint32_t size = 0;
        if (row < nrow)
            for (uint32_t w = tx; w < words32; w += 16) size += (uint32_t)__popc(ref[(size_t)(i0 + row) * words32 + w]);
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) size += (uint32_t)__shfl_xor((int)size, d);
        const uint32_t p = min(size, nleaves - size);
        clamp[x] = p > 0 ? p - 1 : 0;   // (a padding row counts 0 leaves; it is never written)
    }

    for (uint32_t r = blockIdx.y; r < nrep; r += gridDim.y) {
        const uint32_t jbeg = rep_off[r], jend = rep_off[r + 1];
        uint32_t best[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        for (uint32_t j0 = jbeg; j0 < jend;) {
            uint32_t acc[4][4];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] = 0;
            for (uint32_t w0 = 0; w0 < words32; w0 += PGM_TRANSFER_K) {
#pragma unroll 4
                for (uint32_t e = tid; e < PGM_TRANSFER_T * PGM_TRANSFER_K; e += 256) {
                    const uint32_t row = e / PGM_TRANSFER_K, k = e % PGM_TRANSFER_K, w = w0 + k;
                    uint32_t va = 0, vb = 0;   // (a set or a word that does not exist: zero on both sides adds nothing)
                    if (w < words32) {
                        if (row < nrow) va = ref[(size_t)(i0 + row) * words32 + w];
                        if (row < jend - j0) vb = rep[(size_t)(j0 + row) * words32 + w];
                    }
                    sA[k][row] = va;
                    sB[k][row] = vb;
                }
                __syncthreads();
#pragma unroll 2
                for (uint32_t k = 0; k < PGM_TRANSFER_K; ++k) {
                    const uint4 a = *reinterpret_cast<const uint4 *>(&sA[k][ty * 4]);
                    const uint4 b = *reinterpret_cast<const uint4 *>(&sB[k][tx * 4]);
                    const uint32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int y = 0; y < 4; ++y) acc[x][y] += (uint32_t)__popc(av[x] ^ bv[y]);
                }
                __syncthreads();
            }
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                if (tx * 4 + (uint32_t)y >= jend - j0) continue;   // a padding column of a partial tile
#pragma unroll
                for (int x = 0; x < 4; ++x) best[x] = min(best[x], min(acc[x][y], nleaves - acc[x][y]));
            }
            if (jend - j0 <= PGM_TRANSFER_T) break;   // (not j0 += T in the loop head: it could wrap past 2^32)
            j0 += PGM_TRANSFER_T;
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            uint32_t m = best[x];
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, d));
            const uint32_t row = ty * 4 + (uint32_t)x;
            if (tx == 0 && row < nrow) phi[(size_t)(i0 + row) * nrep + r] = min(m, clamp[x]);
        }
    }
}

#endif
