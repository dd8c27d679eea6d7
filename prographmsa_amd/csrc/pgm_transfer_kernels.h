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
//
// pgm_transfer_min_kernel<true> (pgmsa --bootstrap_taxa; pgm_transfer_taxa) also keeps where the minimum is: the running minimum of a
// row is the 64-bit key  d * 2^33 + s * 2 + flip  (s the index of the set in rep, flip = the moved set is the complement of A xor B:
// h > nleaves - h), so the minimum over keys is the lowest d and then the lowest s.  It writes arg[e][r] = s, or
// PGM_TRANSFER_NONE when no set is as near as the clamp p - 1, and flip[e][r] = 0 or ~0, the mask pgm_transfer_moved_kernel applies.
// <false> is the kernel of pgm_transfer_min, unchanged: nothing of the key is compiled into it.
//
// pgm_transfer_moved_kernel: moved[e][t] = the number of counted replicates r (arg != NONE and phi <= thr[e]) whose moved set
// A_e xor B_arg xor flip holds leaf t, and counted[e] = the number of counted r.  A workgroup per reference set (blockIdx.x) and
// leaves t = (blockIdx.y + k gridDim.y) * 256 + lane: the workgroup stages arg and flip of 256 replicates in LDS (NONE for one
// that is not counted), then every thread tests its leaf's bit of the word it shares with 31 neighbours, one independent load per
// counted replicate.  One writer per moved entry and per counted entry: no atomics, nothing zeroed.
#ifndef PGM_TRANSFER_KERNELS_H_
#define PGM_TRANSFER_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGM_TRANSFER_T 64     // sets of a tile, on either side
#define PGM_TRANSFER_K 32     // 32-bit words of one staged chunk
#define PGM_TRANSFER_PAD 68   // words per staged row: 64 sets + 4, keeps 16-byte alignment and spreads the staging stores over the banks
#define PGM_TRANSFER_NOSET 0xffffffffu   // (PGM_TRANSFER_NONE of include/pgm_hip.h)

// grid: (tiles of PGM_TRANSFER_T reference sets, replicate lanes) workgroups of 256; words32 = 2 * ((nleaves + 63) / 64)
// kArg: also arg and flip (nref x nrep each; null and never touched without)
template <bool kArg>
__global__ void __launch_bounds__(256) pgm_transfer_min_kernel(const uint32_t *__restrict__ ref, uint32_t nref, const uint32_t *__restrict__ rep,
                                                               const uint32_t *__restrict__ rep_off, uint32_t nrep, uint32_t nleaves, uint32_t words32,
                                                               uint32_t *__restrict__ phi, uint32_t *__restrict__ arg, uint32_t *__restrict__ flip) {
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
        uint64_t key[4] = {~0ull, ~0ull, ~0ull, ~0ull};   // (kArg: d is below 2^31, so no key of a set reaches this)
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
                for (int x = 0; x < 4; ++x) {
                    if constexpr (kArg) {
                        const uint32_t h = acc[x][y], c = nleaves - h;
                        const uint64_t k = ((uint64_t)min(h, c) << 33) | ((uint64_t)(j0 + tx * 4 + (uint32_t)y) << 1) | (uint64_t)(h > c);
                        key[x] = min(key[x], k);
                    } else {
                        best[x] = min(best[x], min(acc[x][y], nleaves - acc[x][y]));
                    }
                }
            }
            if (jend - j0 <= PGM_TRANSFER_T) break;   // (not j0 += T in the loop head: it could wrap past 2^32)
            j0 += PGM_TRANSFER_T;
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const uint32_t row = ty * 4 + (uint32_t)x;
            if constexpr (kArg) {
                uint64_t k = key[x];
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {   // the key as two 32-bit halves
                    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), d);
                    k = min(k, ((uint64_t)hi << 32) | lo);
                }
                if (tx == 0 && row < nrow) {
                    const size_t o = (size_t)(i0 + row) * nrep + r;
                    const bool reached = (k >> 33) <= clamp[x];   // (else only the clamp gives phi: no set to name)
                    phi[o] = reached ? (uint32_t)(k >> 33) : clamp[x];
                    arg[o] = reached ? (uint32_t)(k >> 1) : PGM_TRANSFER_NOSET;
                    flip[o] = reached && (k & 1) ? 0xffffffffu : 0u;
                }
            } else {
                uint32_t m = best[x];
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, d));
                if (tx == 0 && row < nrow) phi[(size_t)(i0 + row) * nrep + r] = min(m, clamp[x]);
            }
        }
    }
}

// grid: (nref, tiles of 256 leaves up to 65535) workgroups of 256.  rep holds the sets as 32-bit words, as above; arg, flip and phi
// are what pgm_transfer_min_kernel<true> wrote for the same sets.
__global__ void __launch_bounds__(256) pgm_transfer_moved_kernel(const uint32_t *__restrict__ ref, const uint32_t *__restrict__ rep, uint32_t nrep,
                                                                 uint32_t nleaves, uint32_t words32, const uint32_t *__restrict__ thr,
                                                                 const uint32_t *__restrict__ phi, const uint32_t *__restrict__ arg,
                                                                 const uint32_t *__restrict__ flip, uint32_t *__restrict__ moved,
                                                                 uint32_t *__restrict__ counted) {
    __shared__ uint32_t sArg[256], sFlip[256];
    const uint32_t tid = threadIdx.x, e = blockIdx.x, limit = thr[e];
    const size_t row = (size_t)e * nrep;
    for (uint32_t t0 = blockIdx.y * 256u; t0 < nleaves;) {
        const uint32_t t = t0 + tid, w = t >> 5, b = t & 31u;
        const bool leaf = t < nleaves;   // (w < words32 then)
        const uint32_t a = leaf ? ref[(size_t)e * words32 + w] >> b : 0u;
        uint32_t sum = 0, cnt = 0;
        for (uint32_t r0 = 0; r0 < nrep;) {
            const uint32_t m = min(256u, nrep - r0);
            uint32_t s = PGM_TRANSFER_NOSET, f = 0;
            if (tid < m && phi[row + r0 + tid] <= limit) { s = arg[row + r0 + tid]; f = flip[row + r0 + tid]; }
            sArg[tid] = s;
            sFlip[tid] = f;
            __syncthreads();
#pragma unroll 4
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t sk = sArg[k];   // (uniform over the workgroup)
                if (sk == PGM_TRANSFER_NOSET) continue;
                ++cnt;
                if (leaf) sum += ((a ^ (rep[(size_t)sk * words32 + w] >> b)) ^ sFlip[k]) & 1u;
            }
            __syncthreads();
            if (nrep - r0 <= 256u) break;   // (not r0 += 256 in the loop head: it could wrap past 2^32)
            r0 += 256u;
        }
        if (leaf) moved[(size_t)e * nleaves + t] = sum;
        if (t0 == 0 && tid == 0) counted[e] = cnt;   // (blockIdx.y == 0, first tile)
        const uint64_t next = (uint64_t)t0 + (uint64_t)gridDim.y * 256u;
        if (next >= nleaves) break;
        t0 = (uint32_t)next;
    }
}

#endif
