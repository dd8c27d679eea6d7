// pgm_parsimony_kernels.h — the root search's device work (reference src/FindRoot.h, src/GapParsimony.h):
//   pgm_gapmask_extend_kernel   extend_alignment (ProgressiveAlignment.h:245-264) on 1-bit gap masks
//   pgm_gap_parsimony_kernel    GapParsimony::scoreAlignment of many candidate alignments
// Both are integer bit arithmetic: the results are exact.
#ifndef PGM_PARSIMONY_KERNELS_H_
#define PGM_PARSIMONY_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

struct PgmGapmaskJobDev {
    const uint64_t *src;
    const int32_t *rank;     // per merged column: the child column it takes, -1 = gap (the prefix sum of the mapping)
    uint64_t *dst;
    uint32_t nrows, words_in, ncols_out, words_out;
};

// one workgroup per job (grid-stride over the jobs); one lane per (row, output word): the 64 bits are gathered through the
// job's shared rank array
__global__ void __launch_bounds__(256) pgm_gapmask_extend_kernel(const PgmGapmaskJobDev *__restrict__ jobs, uint32_t njobs) {
    for (uint32_t j = blockIdx.x; j < njobs; j += gridDim.x) {
        const PgmGapmaskJobDev J = jobs[j];
        const uint64_t total = (uint64_t)J.nrows * J.words_out;
        for (uint64_t t = threadIdx.x; t < total; t += blockDim.x) {
            const uint32_t row = (uint32_t)(t / J.words_out), w = (uint32_t)(t % J.words_out);
            const uint64_t *src = J.src + (size_t)row * J.words_in;
            uint64_t out = 0;
            const uint32_t c0 = w * 64u, c1 = min(c0 + 64u, J.ncols_out);
            for (uint32_t c = c0; c < c1; ++c) {
                const int32_t r = J.rank[c];
                const uint64_t bit = r < 0 ? 1ull : (src[(uint32_t)r >> 6] >> ((uint32_t)r & 63u)) & 1ull;
                out |= bit << (c - c0);
            }
            J.dst[(size_t)row * J.words_out + w] = out;
        }
    }
}

struct PgmParsimonyJobDev {
    const uint64_t *masks;       // nleaves x words
    const uint32_t *children;    // 2 (nleaves - 1)
    uint32_t nleaves, ncols, words, nblocks;   // nblocks = ceil(ncols / 32): the reference's 64-bit blocks of 32 columns
};

// bit c of x to bit 2c
__device__ __forceinline__ uint64_t pgm_spread32(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// the reference's leaf bitset of block b (GapParsimony.h:36-52): bit 2c residue, bit 2c + 1 gap; the columns of the last block
// from length % 32 on are ones — all 32 of them when the length is a multiple of 32
__device__ __forceinline__ uint64_t pgm_leaf_block(const uint64_t *row, uint32_t b, uint32_t nblocks, uint32_t ncols) {
    const uint32_t g = (uint32_t)(row[b >> 1] >> (32u * (b & 1u)));
    const uint32_t nv = b + 1 < nblocks ? 32u : ncols % 32u;
    const uint32_t vm = nv == 32u ? 0xFFFFFFFFu : (1u << nv) - 1u;
    return pgm_spread32(~g & vm) | (pgm_spread32(g & vm) << 1) | (pgm_spread32(~vm) * 3ull);
}

// One workgroup per candidate (grid-stride over the candidates).  Lane l owns the blocks l, l + 256, ... of every node and walks
// the post-order list; the consensus of internal node k (not the root) goes to the workgroup's scratch region, [k][block], so
// the lanes' accesses are consecutive words.  A lane reads back only its own blocks: no barrier inside the walk.
__global__ void __launch_bounds__(256) pgm_gap_parsimony_kernel(const PgmParsimonyJobDev *__restrict__ jobs, uint32_t njobs,
                                                               uint64_t *__restrict__ scratch, uint64_t scratch_words,
                                                               uint32_t *__restrict__ scores) {
    __shared__ uint32_t total;
    uint64_t *mine = scratch + (size_t)blockIdx.x * scratch_words;
    const uint64_t HI = 0xAAAAAAAAAAAAAAAAull;
    for (uint32_t j = blockIdx.x; j < njobs; j += gridDim.x) {
        const PgmParsimonyJobDev J = jobs[j];
        if (threadIdx.x == 0) total = 0;
        __syncthreads();
        const uint32_t ninner = J.nleaves - 1, NB = J.nblocks;
        uint32_t count = 0;
        for (uint32_t b = threadIdx.x; b < NB; b += blockDim.x) {
            for (uint32_t k = 0; k < ninner; ++k) {
                uint64_t w[2];
                for (int s = 0; s < 2; ++s) {
                    const uint32_t c = J.children[2 * k + s];
                    w[s] = c < J.nleaves ? pgm_leaf_block(J.masks + (size_t)c * J.words, b, NB, J.ncols)
                                         : mine[(size_t)(c - J.nleaves) * NB + b];
                }
                const uint64_t x = w[0] & w[1];
                uint64_t t = ~x;
                t = t & (t << 1) & HI;
                count += (uint32_t)__popcll(t);
                if (k + 1 < ninner) mine[(size_t)k * NB + b] = x | t | (t >> 1);
            }
        }
        atomicAdd(&total, count);
        __syncthreads();
        if (threadIdx.x == 0) scores[j] = total;
        __syncthreads();
    }
}

#endif  // PGM_PARSIMONY_KERNELS_H_
