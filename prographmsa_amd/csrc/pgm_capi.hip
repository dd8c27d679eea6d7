// pgm_capi.hip — host side of the C ABI declared in include/pgm_hip.h (libpgm_hip.so).
// Flattens the caller's graphs into HBM-resident job descriptors and launches the HIP kernels of
// pgm_align_kernels.h / pgm_nw_kernels.h / pgm_csprofile_kernels.h.  No CPU fallback exists: every
// entry point needs a working gfx950 device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <thread>
#include <atomic>
#include <chrono>
#include <queue>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <optional>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>
#include <sys/mman.h>

#include "pgm_align_kernels.h"
#include "pgm_crit_kernels.h"
#include "pgm_nw_kernels.h"
#include "pgm_csprofile_kernels.h"
#include "pgm_dist_kernels.h"
#include "pgm_merge_kernels.h"
#include "pgm_parsimony_kernels.h"
#include "pgm_wls_kernels.h"
#include "pgm_bionj_kernels.h"
#include "pgm_agreement_kernels.h"
#include "pgm_transfer_kernels.h"
#include "pgm_treelik_kernels.h"
#include "pgm_resample_kernels.h"
#include "pgm_pool.h"
#include "pgm_plan.h"
#include "pgm_treelik_check.h"
#include "pgm_treelik_plan.h"
static_assert(kC3Bytes == PGM_C3_BYTES, "pgm_plan.h plans the LDS of a crit3 sweep with PGM_C3_BYTES");

static thread_local std::string g_err;
static int fail(int code, const std::string &m) { g_err = m; return code; }
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            return fail(PGM_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_));            \
    } while (0)

struct PgmNwState;
struct pgm_ctx {
    int device = 0;
    PgmNwState *nw = nullptr;        // the all-pairs stage's two tiles in flight (pgm_nw_capi.inc)
    int nw_per_cu = 0;
    // resident merge results (pgm_merge_profiles_batch_ex): bump allocation over chunks that live until pgm_resident_reset
    // (a guide tree is not balanced: a level-1 graph may wait many levels for its sibling)
    struct ResChunk { uint8_t *p; size_t cap; };
    std::vector<ResChunk> res_chunks;
    size_t res_chunk = 0, res_off = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // the lean kernel runs beside the fill kernel (pgm_lean_kernel)
    hipStream_t stream3 = nullptr;   // ... and so does the band kernel (pgm_band_kernel)
    hipStream_t stream4 = nullptr;   // ... and the fill kernel's launch for the longest chains
    // The big buffers of a destroyed batch are kept for the next one (a progressive alignment issues one batch per tree
    // level: hipMalloc / hipFree of several GB per call would dominate the call).  Slot k holds at most one buffer.
    enum { C_IN, C_WORK, C_CELLS, C_OUT, C_S, C_HOST, C_HIN, C_SMALL, C_SLOTS };   // C_HOST, C_HIN: pinned host memory; C_SMALL: the batch's counters, job descriptors, work list
    void *cache_ptr[C_SLOTS] = {};
    size_t cache_bytes[C_SLOTS] = {};
    hipDeviceProp_t prop;
    float nw_ms = 0, cs_ms = 0, ml_ms = 0, merge_ms = 0, pars_ms = 0, wls_ms = 0;
    uint32_t wls_n = 0, wls_launches = 0;   // the WLS refinement: size of the loaded matrices (0 = none), kernels of the last call
    float bionj_ms = 0;
    float agree_ms = 0;                     // --guidance agreement counts: device time of the last call
    float transfer_ms = 0;                  // --bootstrap_tbe / --bootstrap_taxa transfer entries: device time of the last call
    float treelik_ms = 0;                   // --ml_tree likelihood evaluations and --ml_ancestral: device time of the last call
    float resample_ms = 0;                  // --ml_support sums over resampled columns: device time of the last call
    uint32_t bionj_launches = 0;            // BioNJ: device time and kernels of the last call
    // grow-only scratch buffers of the satellite calls (StageCall): a guide-tree stage issues many calls, hipMalloc / hipFree of
    // up to 2 GB per call would dominate them.  The calls of one context are serial; a slot belongs to the stage named beside it
    // and keeps its buffer between that stage's calls.  (The all-pairs stage has buffers of its own: PgmNwState.)
    enum {
        SC_DIST,                            // the distance entries (pgm_dist_capi.inc), shared among them: SC_DIST + position in
        SC_DIST_END = SC_DIST + 9,          //   the call's buffer list (the longest list, pgm_mldist_batch's, has 9 buffers)
        SC_CS = SC_DIST_END,                // the context-profile batch: SC_CS + position in its buffer list
        SC_CS_END = SC_CS + 8,
        SC_MERGE_OUT = SC_CS_END,           // merged profiles of a call that is not resident
        SC_PARS_IN,                         // gap masks and gap parsimony: input image
        SC_PARS_OUT,                        //   outputs and the parsimony consensus scratch
        SC_WLS_MAT,                         // WLS: the (D, W) matrix of pgm_wls_load, read by every later pgm_wls_pair_sums_batch
        SC_WLS_IN,                          //   job image
        SC_WLS_PART,                        //   block partials
        SC_WLS_OUT,                         //   results
        SC_BIONJ_MAT,                       // BioNJ: D, T, V
        SC_BIONJ_VEC,                       //   sums, column minima, descriptors, index lists, plan
        SC_BIONJ_OUT,                       //   join log + final_d
        SC_AGREE_IN,                        // agreement counts: where
        SC_AGREE_OUT,                       //   res_hits followed by pair_hits
        SC_TRANSFER_REF,                    // pgm_transfer_min and pgm_transfer_taxa (shared): reference sets, rep_off, thresholds
        SC_TRANSFER_REP,                    //   replicate sets
        SC_TRANSFER_OUT,                    //   phi (taxa: phi, arg, flip, moved, counted)
        SC_TREELIK_TREE,                    // tree likelihood, ancestral states, NNI and SPR scores, joint states and samples, all eight entries (shared; pgm_treelik_plan.h has the layouts): children lists, pi, weights, rows
        SC_TREELIK_P,                       //   the matrices
        SC_TREELIK_U,                       //   partials and outside vectors (ancestral: the categories' posteriors in their place)
        SC_TREELIK_G,                       //   per-site ratios and chunk sums (rates: the categories' site values and ratios first)
        SC_TREELIK_OUT,                     //   the outputs
        SC_RESAMPLE_X,                      // sums over resampled columns: x as it arrives
        SC_RESAMPLE_XT,                     //   x transposed, rows padded to the q-tile
        SC_RESAMPLE_COLS,                   //   the replicates' columns
        SC_RESAMPLE_OUT,                    //   the sums
        SC_DEV
    };
    enum {
        SH_PROFILES_OUT,                    // pinned: the profiles of a merge / context-profile call on their way to the caller (shared)
        SC_HOST
    };
    void *sc_dev[SC_DEV] = {};
    size_t sc_dev_bytes[SC_DEV] = {};
    void *sc_host[SC_HOST] = {};      // pinned
    size_t sc_host_bytes[SC_HOST] = {};
    hipEvent_t sc_ev[2] = {nullptr, nullptr};
    // context-profile library resident in HBM
    uint32_t csK = 0, csC = 0;
    double *cs_lprofiles = nullptr, *cs_centre = nullptr, *cs_priors = nullptr;
};

// the library's host threads (flattening and chunked upload of the jobs, staging copies, first touch of pinned blocks)
static pgm_pool::Pool &lib_pool() {
    static pgm_pool::Pool pool(std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    return pool;
}

// ---- pinned host blocks ---------------------------------------------------------------------------
// hipHostMalloc of the staging block of a 128-job level (76 MB) takes 10-14 ms in a cold process and stalls every other
// thread that touches the address space meanwhile (hipHostFree: another 8 ms).  A 2 MB aligned block with MADV_HUGEPAGE,
// first touched by a few threads and registered afterwards, is pinned in ~1 ms (tools/micro/pin_bench.hip: fill 0.9 ms,
// hipHostRegister 0.2 ms, same copy rate).  Blocks that could not be registered fall back to hipHostMalloc.
static std::mutex g_pinned_mu;
static std::unordered_set<void *> g_pinned_registered;
static hipError_t pinned_alloc(size_t bytes, void **out) {
    const size_t H = (size_t)2 << 20, len = (std::max<size_t>(bytes, 1) + H - 1) / H * H;
    void *p = getenv("PGM_PINNED_MALLOC") ? nullptr : aligned_alloc(H, len);
    if (p) {
        (void)madvise(p, len, MADV_HUGEPAGE);
        (void)lib_pool().run(len / H, len >= 8 * H ? 16u : 1u, [&](size_t c) { for (size_t o = 0; o < H; o += 4096) ((volatile char *)p)[c * H + o] = 0; });
        if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
            std::lock_guard<std::mutex> g(g_pinned_mu);
            g_pinned_registered.insert(p);
            *out = p;
            return hipSuccess;
        }
        (void)hipGetLastError();
        free(p);
    }
    return hipHostMalloc(out, bytes, hipHostMallocDefault);
}
static void pinned_free(void *p) {
    if (!p) return;
    bool reg;
    { std::lock_guard<std::mutex> g(g_pinned_mu); reg = g_pinned_registered.erase(p) != 0; }
    if (reg) { (void)hipHostUnregister(p); free(p); }
    else (void)hipHostFree(p);
}
static void slot_free(int slot, void *p) {
    if (slot == pgm_ctx::C_HIN) pinned_free(p);
    else if (slot == pgm_ctx::C_HOST) (void)hipHostFree(p);
    else (void)hipFree(p);
}

struct pgm_align_batch {
    uint32_t njobs = 0;
    uint64_t cells = 0;
    uint32_t maxdim = 0, maxnb = 0, maxn = 0, maxnblk = 0;
    std::vector<PgmJob> jobs;         // host copy of the descriptors (device pointers inside)
    std::vector<uint32_t> order;      // launch order: largest job first
    BatchSchedule sched;              // the work lists, their split over the launches and every launch's workers (plan_schedule)
    uint8_t *d_in = nullptr;          // uploaded inputs (arena image)
    uint8_t *d_work = nullptr;        // prep outputs, brow, maps, results, scratch
    uint8_t *d_cells = nullptr;       // DP storage
    uint8_t *d_out = nullptr;         // device working copy of results + mappings (the walk pushes them in reverse order)
    uint8_t *d_S = nullptr;           // emission scores in fill order
    uint8_t *d_small = nullptr;       // d_sync, d_jobs, d_order and the work lists live in this one cached allocation (no hipMalloc / hipFree per batch)
    size_t in_bytes = 0, work_bytes = 0, cell_bytes = 0, out_bytes = 0, s_bytes = 0, small_bytes = 0;
    size_t cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // real sizes of the buffers taken from the context's cache
    uint8_t *h_out = nullptr;          // pinned result block, same layout: written by the kernel itself, read by fetch
    uint8_t *h_in = nullptr;           // pinned staging buffer of the flattened inputs (one H2D copy per create)
    int *h_flag = nullptr;            // (inside h_out, after the results)
    int *d_sync = nullptr;            // [0] abort flag, [1] band-list ticket, then the per-band progress counters of every job
    size_t sync_ints = 0;
    uint32_t lq_off = 0;              // pre-link announcements inside d_sync
    PgmJob *d_jobs = nullptr;
    uint32_t *d_order = nullptr;
    PgmItem *d_items = nullptr;       // sched.items (fill work queue)
    uint32_t *d_lean = nullptr;       // sched.lean_list (pgm_lean_kernel's work queue)
    PgmItem *d_bands = nullptr;       // sched.bands (pgm_band_kernel's work queue)
    int2 *d_tblist = nullptr;         // sched.tblist (the job lists of the instances of pgm_tb_kernel)
    unsigned long long *d_times = nullptr;   // per job {last band complete, traceback published}, then the launch's start (ticks of 10 ns)
    int *d_tabhdr = nullptr;   // class headers of the lean jobs (PgmJob::tabhdr), PGM_TAB_HDR ints per job of the batch; NULL: no lean job
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // stream -> stream2 after the emission kernel, stream2 -> stream after the lean kernel
    hipEvent_t ev_join_b = nullptr, ev_join_c = nullptr;   // ... after the band kernel and the launch of the longest chains (and their tracebacks)
    uint32_t test_spin_limit = 0, test_stall_job = 0xFFFFFFFFu, test_stall_band = 0;   // pgm_align_batch_test_stall
    double acc_ms[3] = {0, 0, 0};     // device time of prep / emission / fill (+ lean kernel + tracebacks) summed over the launches fetched since the last reset
    uint32_t acc_n = 0;
    bool ev_pending = false;          // the last launch recorded its stage events and they have not been read yet
    std::vector<size_t> res_off, map1_off, map2_off;  // offsets inside d_out
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};
// The device buffers of a batch, kept in the context's cache between batches: the cache slot, what pgm_ctx_create reserves for it
// (MB), the batch's pointer and the bytes it needs (the order of the reserve, of the allocation thread and of the "device buffers:" line).
static const struct BatchBuffer { int slot; size_t reserve_mb; uint8_t *pgm_align_batch::*ptr; size_t pgm_align_batch::*bytes; } kBatchBuffers[6] = {
    {pgm_ctx::C_IN, 128, &pgm_align_batch::d_in, &pgm_align_batch::in_bytes}, {pgm_ctx::C_WORK, 256, &pgm_align_batch::d_work, &pgm_align_batch::work_bytes},
    {pgm_ctx::C_CELLS, 2048, &pgm_align_batch::d_cells, &pgm_align_batch::cell_bytes}, {pgm_ctx::C_OUT, 8, &pgm_align_batch::d_out, &pgm_align_batch::out_bytes},
    {pgm_ctx::C_S, 1024, &pgm_align_batch::d_S, &pgm_align_batch::s_bytes}, {pgm_ctx::C_SMALL, 4, &pgm_align_batch::d_small, &pgm_align_batch::small_bytes}};

extern "C" {

const char *pgm_last_error(void) { return g_err.c_str(); }

int pgm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// (launched once per context: the device code of the library is loaded when the context is created, not in the middle of
// the first batch)
__global__ void pgm_warm_kernel() {}

int pgm_ctx_create(int device, pgm_ctx **out) {
    if (!out) return fail(PGM_ERR_INVALID, "null out");
    *out = nullptr;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(PGM_ERR_DEVICE, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    pgm_ctx *c = new pgm_ctx;
    c->device = device;
    HIPCHK(hipGetDeviceProperties(&c->prop, device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
    {   // (the launch of the longest chains on the highest stream priority the device offers)
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
        if (hipStreamCreateWithPriority(&c->stream4, hipStreamNonBlocking, hi) != hipSuccess) {   // (no priorities: an ordinary stream)
            (void)hipGetLastError();
            HIPCHK(hipStreamCreateWithFlags(&c->stream4, hipStreamNonBlocking));
        }
    }
    hipLaunchKernelGGL(pgm_warm_kernel, dim3(1), dim3(64), 0, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    {   // ... and so is the copy path: the first host-to-device copy of a process takes ~8 ms longer than any later one
        void *h = nullptr, *d = nullptr;
        const size_t wb = (size_t)1 << 20;
        if (hipHostMalloc(&h, wb, hipHostMallocDefault) == hipSuccess && hipMalloc(&d, wb) == hipSuccess) {
            (void)hipMemcpyAsync(d, h, wb, hipMemcpyHostToDevice, c->stream);
            (void)hipMemcpyAsync(h, d, wb, hipMemcpyDeviceToHost, c->stream);
            (void)hipStreamSynchronize(c->stream);
        }
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
    }
    // ... and the library's host threads (flattening, staging copies, first touch of pinned blocks): sixteen thread starts are 0.4 ms
    // of whatever call needs them first
    (void)lib_pool().run(64, 16u, [](size_t) {});
    {   // ... and a first staging block for the inputs of a batch in the context's cache (128 MB: a level of 128 jobs of 1000 x 1000
        // takes 37, one of 512 jobs of 600 x 600 95; a larger batch replaces it — 4 ms for the release of a pinned block): allocating, touching and registering it is 0.8-1 ms of the first batch otherwise
        void *p = nullptr;
        const size_t sb = (size_t)128 << 20;
        if (!getenv("PGM_NO_STAGING_RESERVE") && pinned_alloc(sb, &p) == hipSuccess) { c->cache_ptr[pgm_ctx::C_HIN] = p; c->cache_bytes[pgm_ctx::C_HIN] = sb; }
        else (void)hipGetLastError();
        // (and for the results the kernels write over PCIe: 8 MB hold the mappings of 128 jobs of 1000 x 1000 four times over)
        const size_t rb = (size_t)8 << 20;
        if (!getenv("PGM_NO_STAGING_RESERVE") && hipHostMalloc(&p, rb, hipHostMallocDefault) == hipSuccess) { c->cache_ptr[pgm_ctx::C_HOST] = p; c->cache_bytes[pgm_ctx::C_HOST] = rb; }
        else (void)hipGetLastError();
        // The device side of the same cache: 3.4 GB of the 288 (inputs 128 MB, prep outputs / codes 256 MB, DP cells 2 GB, results 8 MB,
        // emission scores 1 GB, descriptors 4 MB) — what the levels of a 256 x 1000 or a 1024 x 600 pass take; a larger batch replaces a block.  On
        // most hosts of the pool these six hipMalloc calls take 0.3 ms together; on some (or in some states of a host) the driver
        // hands out device memory at ~30 ms per GB, and the first two levels of a pass then waited 50-70 ms for their buffers
        // (DESIGN section 4): a runtime pays that when it starts, not in the middle of its first call.  PGM_NO_DEVICE_RESERVE=1: off.
        if (!getenv("PGM_NO_STAGING_RESERVE") && !getenv("PGM_NO_DEVICE_RESERVE")) {
            for (const BatchBuffer &e : kBatchBuffers) {
                void *d = nullptr;
                if (hipMalloc(&d, e.reserve_mb << 20) == hipSuccess) { c->cache_ptr[e.slot] = d; c->cache_bytes[e.slot] = e.reserve_mb << 20; }
                else { (void)hipGetLastError(); break; }
            }
        }
    }
    *out = c;
    return PGM_OK;
}

static void nw_state_free(PgmNwState *st);
void pgm_ctx_destroy(pgm_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    nw_state_free(ctx->nw);
    for (auto &c : ctx->res_chunks) if (c.p) (void)hipFree(c.p);
    if (ctx->cs_lprofiles) (void)hipFree(ctx->cs_lprofiles);
    if (ctx->cs_centre) (void)hipFree(ctx->cs_centre);
    if (ctx->cs_priors) (void)hipFree(ctx->cs_priors);
    for (int k = 0; k < pgm_ctx::SC_DEV; ++k) if (ctx->sc_dev[k]) (void)hipFree(ctx->sc_dev[k]);
    for (int k = 0; k < pgm_ctx::SC_HOST; ++k) if (ctx->sc_host[k]) pinned_free(ctx->sc_host[k]);
    for (int k = 0; k < 2; ++k) if (ctx->sc_ev[k]) (void)hipEventDestroy(ctx->sc_ev[k]);
    for (int k = 0; k < pgm_ctx::C_SLOTS; ++k)
        if (ctx->cache_ptr[k]) slot_free(k, ctx->cache_ptr[k]);
    if (ctx->stream4) (void)hipStreamDestroy(ctx->stream4);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int pgm_ctx_device_info(pgm_ctx *ctx, char *name, size_t name_len, int *cu_count) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null ctx");
    if (name && name_len) snprintf(name, name_len, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (cu_count) *cu_count = ctx->prop.multiProcessorCount;
    return PGM_OK;
}

}  // extern "C"

namespace {
// take a buffer of at least `bytes` from the context's cache slot, or allocate one (device memory; slot C_HOST: pinned host)
static hipError_t cache_take(pgm_ctx *ctx, int slot, size_t bytes, void **out, size_t *got) {
    if (ctx->cache_ptr[slot] && ctx->cache_bytes[slot] >= bytes) {
        *out = ctx->cache_ptr[slot]; *got = ctx->cache_bytes[slot];
        ctx->cache_ptr[slot] = nullptr; ctx->cache_bytes[slot] = 0;
        return hipSuccess;
    }
    if (ctx->cache_ptr[slot]) {   // too small: replace
        slot_free(slot, ctx->cache_ptr[slot]);
        ctx->cache_ptr[slot] = nullptr; ctx->cache_bytes[slot] = 0;
    }
    *got = bytes;
    if (slot == pgm_ctx::C_HIN) return pinned_alloc(bytes, out);
    return slot == pgm_ctx::C_HOST ? hipHostMalloc(out, bytes, hipHostMallocDefault) : hipMalloc(out, bytes);
}
static void cache_give(pgm_ctx *ctx, int slot, void *p, size_t bytes) {
    if (!p) return;
    if (ctx && (!ctx->cache_ptr[slot] || ctx->cache_bytes[slot] < bytes)) {
        if (ctx->cache_ptr[slot]) slot_free(slot, ctx->cache_ptr[slot]);
        ctx->cache_ptr[slot] = p; ctx->cache_bytes[slot] = bytes;
    } else {
        slot_free(slot, p);
    }
}

// scratch buffer `slot` of the context with room for `bytes` (device memory, or pinned host memory)
static hipError_t scratch_dev(pgm_ctx *ctx, int slot, size_t bytes, void **out) {
    bytes = std::max<size_t>(bytes, 16);
    if (ctx->sc_dev_bytes[slot] < bytes) {
        if (ctx->sc_dev[slot]) (void)hipFree(ctx->sc_dev[slot]);
        ctx->sc_dev[slot] = nullptr; ctx->sc_dev_bytes[slot] = 0;
        const size_t want = bytes + bytes / 4;
        hipError_t e = hipMalloc(&ctx->sc_dev[slot], want);
        if (e != hipSuccess) return e;
        ctx->sc_dev_bytes[slot] = want;
    }
    *out = ctx->sc_dev[slot];
    return hipSuccess;
}
static hipError_t scratch_host(pgm_ctx *ctx, int slot, size_t bytes, void **out) {
    bytes = std::max<size_t>(bytes, 16);
    if (ctx->sc_host_bytes[slot] < bytes) {
        if (ctx->sc_host[slot]) pinned_free(ctx->sc_host[slot]);
        ctx->sc_host[slot] = nullptr; ctx->sc_host_bytes[slot] = 0;
        const size_t want = bytes + bytes / 4;
        hipError_t e = pinned_alloc(want, &ctx->sc_host[slot]);
        if (e != hipSuccess) return e;
        ctx->sc_host_bytes[slot] = want;
    }
    *out = ctx->sc_host[slot];
    return hipSuccess;
}
static hipError_t scratch_events(pgm_ctx *ctx) {
    for (int k = 0; k < 2; ++k)
        if (!ctx->sc_ev[k]) { hipError_t e = hipEventCreate(&ctx->sc_ev[k]); if (e != hipSuccess) return e; }
    return hipSuccess;
}

// `bytes` of the context's resident memory (bump allocation over chunks, in steps of 256 bytes): valid until pgm_resident_reset
static hipError_t resident_alloc(pgm_ctx *ctx, size_t bytes, uint8_t **out) {
    bytes = (bytes + 255) / 256 * 256;
    while (ctx->res_chunk < ctx->res_chunks.size() && ctx->res_off + bytes > ctx->res_chunks[ctx->res_chunk].cap) { ++ctx->res_chunk; ctx->res_off = 0; }
    if (ctx->res_chunk == ctx->res_chunks.size()) {
        pgm_ctx::ResChunk c{nullptr, std::max<size_t>(bytes, (size_t)96 << 20)};
        const hipError_t e = hipMalloc((void **)&c.p, c.cap);
        if (e != hipSuccess) return e;
        ctx->res_chunks.push_back(c); ctx->res_off = 0;
    }
    *out = ctx->res_chunks[ctx->res_chunk].p + ctx->res_off;
    ctx->res_off += bytes;
    return hipSuccess;
}

// The inputs of a call packed into one host image for one upload; put() returns the offset of its block (a multiple of `align`).
struct HostImage {
    size_t align;
    std::vector<uint8_t> bytes;
    explicit HostImage(size_t a = 256) : align(a) {}
    size_t put(const void *src, size_t n) {
        const size_t o = bytes.size();
        bytes.resize(o + (n + align - 1) / align * align);
        if (src && n) memcpy(bytes.data() + o, src, n);   // (src NULL: room only, filled in later)
        return o;
    }
};

// A device buffer of a call whose scratch slot is its place in the call's list (StageCall::bufs).  src: uploaded before the launch;
// dst: copied back behind it; zero: cleared before it.
struct Buf { void **p; size_t bytes; const void *src; void *dst; bool zero; };

// One satellite call on the context's stream — every C entry but the all-pairs stage and the align batch: scratch buffers, uploads,
// the launches between the two events of the stage's timer, the copies back, one synchronisation.  Every method does nothing after
// the first error.  finish() synchronises the stream whenever something was queued, after a failure too: the queued copies read
// and write host memory of the call (its locals, the caller's arrays), so no entry returns before them.
struct StageCall {
    pgm_ctx *ctx;
    const char *what;   // opens the message of a device failure
    float *ms;          // the stage's timer (NULL: none)
    hipStream_t s;
    hipError_t e;
    bool alloc_failed = false, queued = false, timed = false;
    StageCall(pgm_ctx *c, const char *w, float *t) : ctx(c), what(w), ms(t), s(c->stream), e(hipSetDevice(c->device)) {}
    bool ok() const { return e == hipSuccess; }
    // the result of an allocation (PGM_ERR_NOMEM comes from these alone)
    void alloc(hipError_t r) { e = r; alloc_failed = r != hipSuccess; }
    template <class T> void buf(int slot, size_t bytes, T **p) { if (ok()) alloc(scratch_dev(ctx, slot, bytes, (void **)p)); }
    template <class T> void host(int slot, size_t bytes, T **p) { if (ok()) alloc(scratch_host(ctx, slot, bytes, (void **)p)); }
    template <class T> void resident(size_t bytes, T **p) { if (ok()) alloc(resident_alloc(ctx, bytes, (uint8_t **)p)); }
    void up(void *dst, const void *src, size_t bytes) { if (ok() && bytes) { queued = true; e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); } }
    void zero(void *dst, size_t bytes) { if (ok() && bytes) { queued = true; e = hipMemsetAsync(dst, 0, bytes, s); } }
    void down(void *dst, const void *src, size_t bytes) { if (ok() && bytes) { queued = true; e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); } }
    // the buffers of a list in the slots [first, end): taken and, where they have a source, uploaded in the list's order
    void bufs(int first, int end, std::initializer_list<Buf> list) {
        if (ok() && (size_t)(end - first) < list.size()) e = hipErrorInvalidValue;   // (a list longer than its range of pgm_ctx's slot table)
        for (const Buf &b : list) { buf(first++, b.bytes, b.p); if (b.src) up(*b.p, b.src, b.bytes); }
    }
    // begin() ... launches ... end(): the two events of the timer; true: launch
    bool begin() {
        if (ok()) e = scratch_events(ctx);
        if (ok()) { queued = true; e = hipEventRecord(ctx->sc_ev[0], s); }
        return ok();
    }
    void end() {
        if (ok()) e = hipGetLastError();
        if (ok()) e = hipEventRecord(ctx->sc_ev[1], s);
        timed = ok();
    }
    int finish() {
        if (queued) { const hipError_t es = hipStreamSynchronize(s); if (ok()) e = es; }
        if (ok() && timed && ms) (void)hipEventElapsedTime(ms, ctx->sc_ev[0], ctx->sc_ev[1]);
        if (ok()) return PGM_OK;
        (void)hipGetLastError();
        return fail(alloc_failed && e == hipErrorOutOfMemory ? PGM_ERR_NOMEM : PGM_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    }
};

// classes of the nodes of the lean jobs (PgmJob::cls1): once per batch, behind the upload of the inputs and the job descriptors
static hipError_t classify_lean_jobs(pgm_ctx *ctx, pgm_align_batch *b) {
    if (!b->d_tabhdr || b->njobs == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(b->d_tabhdr, 0, 4 * (size_t)PGM_TAB_HDR * b->njobs, ctx->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pgm_classify_kernel, dim3(b->njobs, 2, (b->maxn + 1023) / 1024), dim3(256), 0, ctx->stream, b->d_jobs);
    return hipGetLastError();
}

#define PGM_STATUS_PENDING 0x7ffffff0   /* status word of a job's result record in the pinned block until its traceback worker has written it */
// the instantiation of the prep and emission kernels for a batch's largest alphabet (alphabet_tier, as for the jobs' dp), the prep
// kernel's block size and its LDS
struct PrepTier { uint32_t tier, threads; size_t lds; };
static PrepTier prep_tier(uint32_t maxdim) {
    const uint32_t tier = alphabet_tier(maxdim), threads = tier == 64u ? 64u : 256u;
    return {tier, threads, ((size_t)maxdim * maxdim + maxdim + threads * ((size_t)maxdim + 1)) * sizeof(float)};
}
static hipError_t launch_all(pgm_ctx *ctx, pgm_align_batch *b, bool timed) {
    hipStream_t s = ctx->stream;
    const BatchSchedule &S = b->sched;
    hipError_t e;
    for (uint32_t i = 0; i < b->njobs; ++i) ((PgmJob::Result *)(b->h_out + b->res_off[i]))->status = PGM_STATUS_PENDING;
    if (timed && (e = hipEventRecord(b->ev[0], s)) != hipSuccess) return e;
    const PrepTier T = prep_tier(b->maxdim);
    const dim3 pg(b->njobs, 2, (b->maxn + T.threads - 1) / T.threads);
    if (T.tier == 4) hipLaunchKernelGGL((pgm_prep_kernel<4, 256>), pg, dim3(256), T.lds, s, b->d_jobs, b->d_sync, (uint32_t)b->sync_ints);
    else if (T.tier == 20) hipLaunchKernelGGL((pgm_prep_kernel<20, 256>), pg, dim3(256), T.lds, s, b->d_jobs, b->d_sync, (uint32_t)b->sync_ints);
    else hipLaunchKernelGGL((pgm_prep_kernel<64, 64>), pg, dim3(64), T.lds, s, b->d_jobs, b->d_sync, (uint32_t)b->sync_ints);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(b->ev[1], s)) != hipSuccess) return e;
    // (RB = 2 bands per thread — one LDS read of a column pair for four cells — was measured at half the speed: 0.55 -> 1.13 ms)
    const dim3 eg((b->maxnblk + PGM_EM_TB - 1) / PGM_EM_TB, (b->maxnb + 3) / 4, b->njobs);
    if (T.tier == 4) hipLaunchKernelGGL((pgm_emission_skew_kernel<4, 1>), eg, dim3(4 * PGM_ROWS), 0, s, b->d_jobs);
    else if (T.tier == 20) hipLaunchKernelGGL((pgm_emission_skew_kernel<20, 1>), eg, dim3(4 * PGM_ROWS), 0, s, b->d_jobs);
    else hipLaunchKernelGGL((pgm_emission_skew_kernel<64, 1>), eg, dim3(4 * PGM_ROWS), 0, s, b->d_jobs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(b->ev[2], s)) != hipSuccess) return e;
    // The sweep kernels, then the traceback kernel behind each of them on its stream.
    // test knobs for the hand-off time-out path (tests/test_gpu_align.py): a shorter spin limit, and one band of one job
    // that never publishes its progress ("job:band"), so that the band below it times out and the batch aborts
    const uint32_t spin_limit = b->test_spin_limit ? b->test_spin_limit : PGM_SPIN_LIMIT, stall_job = b->test_stall_job, stall_band = b->test_stall_band;   // (pgm_align_batch_test_stall)
    const bool fork = S.nlean != 0;
    const bool bandk = S.nbands != 0;
    const bool tbk = (S.nitems != 0 || bandk) && (S.ntb + S.ntb_c + S.ntb_b) != 0;   // the traceback kernel behind the sweep kernels
    const bool critk = S.ncrit != 0;
    if ((fork || bandk || critk) && (e = hipEventRecord(b->ev_fork, s)) != hipSuccess) return e;
    if (critk && (e = hipStreamWaitEvent(ctx->stream4, b->ev_fork, 0)) != hipSuccess) return e;
    if (fork && (e = hipStreamWaitEvent(ctx->stream2, b->ev_fork, 0)) != hipSuccess) return e;
    if (bandk && (e = hipStreamWaitEvent(ctx->stream3, b->ev_fork, 0)) != hipSuccess) return e;
    const uint32_t nrest = S.nitems - S.ncrit;
    // The launch of the longest chains goes out on the PRIMARY stream, right behind the emission kernel; the main launch on stream4, behind
    // the fork event like the lean and band kernels (a kernel behind an event of another stream starts 50-60 us later: measured on the
    // root of the headline batch, whose traceback is the last thing the stage waits for, when it was the other way round).
    hipStream_t sc = critk ? s : ctx->stream4, sr = critk ? ctx->stream4 : s;
    // a part of the work list, swept by pgm_crit_kernel (every item of it belongs to a crit3 job) or by pgm_fill_kernel
    auto sweep = [&](hipStream_t st, uint32_t workers, const PgmItem *list, uint32_t n, bool c3, uint32_t ticket_off) {
        if (c3) hipLaunchKernelGGL(pgm_crit_kernel, dim3(workers), dim3(64 * PGM_C3_WAVES), 0, st, b->d_jobs, list, n, b->d_sync, spin_limit, stall_job, stall_band, ticket_off);
        else hipLaunchKernelGGL(pgm_fill_kernel, dim3(workers), dim3(64 * PGM_WAVES), 0, st, b->d_jobs, list, n, b->d_sync, spin_limit, stall_job, stall_band, ticket_off);
    };
    // the tracebacks of the jobs tblist[first, first + n), behind their sweep kernel on its stream and its CUs
    auto tracebacks = [&](hipStream_t st, uint32_t workers, uint32_t first, uint32_t n, uint32_t lq_off, uint32_t sybase) {
        hipLaunchKernelGGL(pgm_tb_kernel, dim3(workers), dim3(64 * PGM_WAVES), 0, st, b->d_jobs, b->d_tblist + first, n, b->d_sync, b->test_spin_limit, lq_off, sybase, 1u);
    };
    if (critk) sweep(sc, S.ncrit_workers, b->d_items, S.ncrit, S.crit_c3, (uint32_t)PGM_SY_CRIT_TICKET);
    if (nrest != 0) sweep(sr, S.nworkers, b->d_items + S.ncrit, nrest, S.rest_c3, 1u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (fork) {
        // the lean jobs' kernel, launched after the fill kernel (whose grid leaves nlean_workers CUs free)
        hipLaunchKernelGGL((pgm_lean_kernel<2>), dim3(S.nlean_workers), dim3(64 * PGM_WAVES), 0, ctx->stream2, b->d_jobs, b->d_lean, S.nlean, b->d_sync, spin_limit);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const uint32_t njp = (b->njobs + 3u) / 4u * 4u;
    if (bandk) {
        // the bands of the MODE 0 / 1 jobs, one per wavefront, on their share of the CUs; their tracebacks follow on the same
        // stream and the same CUs (the band queue is done well before the chains of the fill kernel are)
        hipLaunchKernelGGL(pgm_band_kernel, dim3(S.nband_workers), dim3(64 * PGM_WAVES), 0, ctx->stream3, b->d_jobs, b->d_bands, S.nbands_narrow, S.nbands, S.nband_workers - S.nwide_workers, b->d_sync, spin_limit, stall_job, stall_band);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (tbk && S.ntb_b) tracebacks(ctx->stream3, S.ntb_b_workers, S.ntb + S.ntb_c, S.ntb_b, b->lq_off + njp, 8u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(b->ev_join_b, ctx->stream3)) != hipSuccess) return e;
    }
    if (critk) {
        if (tbk && S.ntb_c) tracebacks(sc, S.ncrit_workers, S.ntb, S.ntb_c, b->lq_off + 2 * njp, 16u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (tbk && S.ntb) {
        // the tracebacks of the fill kernel's jobs, behind it on its stream
        tracebacks(sr, S.ntb_workers, 0u, S.ntb, b->lq_off, 0u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (critk && (e = hipEventRecord(b->ev_join_c, ctx->stream4)) != hipSuccess) return e;   // (behind whatever went to stream4)
    if (bandk && (e = hipStreamWaitEvent(s, b->ev_join_b, 0)) != hipSuccess) return e;
    if (critk && (e = hipStreamWaitEvent(s, b->ev_join_c, 0)) != hipSuccess) return e;
    if (fork && ((e = hipEventRecord(b->ev_join, ctx->stream2)) != hipSuccess || (e = hipStreamWaitEvent(s, b->ev_join, 0)) != hipSuccess)) return e;
    if (timed && (e = hipEventRecord(b->ev[3], s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(b->ev[4], s)) != hipSuccess) return e;
    return hipSuccess;
}
// ---- the phases of pgm_align_batch_create_res ------------------------------------------------------
// one small allocation: progress counters, job descriptors, size order, work lists (at most one item per band), job times, class headers
struct SmallLayout { size_t sync, jobs, order, items, lean, tblist, bands, times, tabhdr, total_bands; bool any_lean; };
static SmallLayout layout_small(pgm_align_batch *b) {
    SmallLayout s;
    const uint32_t njobs = b->njobs;
    s.total_bands = 0; s.any_lean = false;
    for (const PgmJob &J : b->jobs) { s.total_bands += J.nb; s.any_lean = s.any_lean || (J.lean && !J.keep_cells); }
    DevLayout SM;
    s.sync = SM.take(b->sync_ints * sizeof(int)); s.jobs = SM.take(sizeof(PgmJob) * std::max(1u, njobs));
    s.order = SM.take(4 * (size_t)std::max(1u, njobs)); s.items = SM.take(sizeof(PgmItem) * std::max<size_t>(1, s.total_bands));
    s.lean = SM.take(4 * (size_t)std::max(1u, njobs)); s.tblist = SM.take(8 * (size_t)std::max(1u, njobs));
    s.bands = SM.take(sizeof(PgmItem) * std::max<size_t>(1, s.total_bands)); s.times = SM.take(16 * (size_t)std::max(1u, njobs) + 16);
    s.tabhdr = SM.take(s.any_lean ? 4 * (size_t)PGM_TAB_HDR * njobs : 16);
    b->small_bytes = SM.bytes;
    return s;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What the allocation thread reports.  The device buffers and the pinned result block are allocated (or taken from the context's
// cache) on a thread of their own while the jobs are being flattened: all sizes are known after pass 1.
struct BatchAlloc {
    std::atomic<int> state{0};   // 1: the device buffers exist (the flattening threads then upload their jobs' slices), -1: failed
    hipError_t err = hipSuccess, host_err = hipSuccess;
    uint8_t *h_out_dev = nullptr;
    double ms_dev = 0, ms_host = 0, ms_slot[6] = {0, 0, 0, 0, 0, 0};
};
static void take_batch_buffers(pgm_ctx *ctx, pgm_align_batch *b, SmallLayout sm, BatchAlloc *A) {
    const double ta0 = now_ms();
    hipError_t e2 = hipSetDevice(ctx->device);
    double tprev = ta0;
    for (int k = 0; k < 6 && e2 == hipSuccess; ++k) {
        const BatchBuffer &s = kBatchBuffers[k];
        e2 = cache_take(ctx, s.slot, b->*s.bytes, (void **)&(b->*s.ptr), &b->cap[s.slot]);
        const double t = now_ms(); A->ms_slot[k] = t - tprev; tprev = t;
    }
    if (e2 == hipSuccess) {
        b->d_sync = (int *)(b->d_small + sm.sync);
        b->d_jobs = (PgmJob *)(b->d_small + sm.jobs);
        b->d_order = (uint32_t *)(b->d_small + sm.order);
        b->d_items = (PgmItem *)(b->d_small + sm.items);
        b->d_lean = (uint32_t *)(b->d_small + sm.lean);
        b->d_tblist = (int2 *)(b->d_small + sm.tblist);
        b->d_bands = (PgmItem *)(b->d_small + sm.bands);
        b->d_times = (unsigned long long *)(b->d_small + sm.times);
        b->d_tabhdr = sm.any_lean ? (int *)(b->d_small + sm.tabhdr) : nullptr;
    }
    A->err = e2;
    A->state.store(e2 == hipSuccess ? 1 : -1, std::memory_order_release);
    A->ms_dev = now_ms() - ta0;
    // pinned result block, same layout as d_out: the traceback workers write the finished mappings and result records
    // into it over PCIe while the kernel is still running
    if (e2 == hipSuccess) {
        hipError_t e3 = cache_take(ctx, pgm_ctx::C_HOST, b->out_bytes + 64, (void **)&b->h_out, &b->cap[pgm_ctx::C_HOST]);
        if (e3 == hipSuccess) b->h_flag = (int *)(b->h_out + (b->out_bytes + 15) / 16 * 16);
        if (e3 == hipSuccess) e3 = hipHostGetDevicePointer((void **)&A->h_out_dev, b->h_out, 0);
        A->host_err = e3;
    }
    A->ms_host = now_ms() - ta0 - A->ms_dev;
}

// Whatever ends pgm_align_batch_create_res early: the allocation thread is joined, then the batch is destroyed (its buffers go
// back to the context's cache).  release() hands the finished batch to the caller.
struct CreateGuard {
    pgm_ctx *ctx;
    pgm_align_batch *b;
    std::thread alloc;
    ~CreateGuard() { if (alloc.joinable()) alloc.join(); if (b) pgm_align_batch_destroy(ctx, b); }
    pgm_align_batch *release() { pgm_align_batch *r = b; b = nullptr; return r; }
};

// the offsets of pass 1 as device pointers of the job descriptors
static void bind_job_pointers(pgm_align_batch *b, const std::vector<JobOff> &off, const pgm_site_ref *res1, const pgm_site_ref *res2, uint8_t *h_out_dev) {
    for (uint32_t i = 0; i < b->njobs; ++i) {
        PgmJob &J = b->jobs[i];
        const JobOff &o = off[i];
        uint8_t *in = b->d_in, *w = b->d_work, *ob = b->d_out;
        J.sites1 = site_ref_of(res1, i) ? res1[i].dev_sites : (const double *)(in + o.s1.sites);
        J.sites2 = site_ref_of(res2, i) ? res2[i].dev_sites : (const double *)(in + o.s2.sites);
        J.smap1 = o.s1.has_smap ? (const uint32_t *)(in + o.s1.smap) : nullptr;
        J.smap2 = o.s2.has_smap ? (const uint32_t *)(in + o.s2.smap) : nullptr;
        J.M = (const double *)(in + o.M); J.pi = (const double *)(in + o.pi);
        J.ni1 = (const PgmNode2 *)(in + o.s1.ni); J.ni2 = (const PgmNode2 *)(in + o.s2.ni);
        J.xp1 = (const int32_t *)(in + o.s1.xp); J.xp2 = (const int32_t *)(in + o.s2.xp);
        J.xc1 = (const uint32_t *)(in + o.s1.xc); J.xc2 = (const uint32_t *)(in + o.s2.xc);
        J.xv1 = (const float *)(in + o.s1.xv); J.xv2 = (const float *)(in + o.s2.xv);
        J.fp1 = (const int32_t *)(in + o.s1.fp); J.fe1 = (const uint2 *)(in + o.s1.fe);
        J.ov2 = (const uint2 *)(in + o.s2.ov);
        J.pp1 = (const int32_t *)(in + o.s1.pp); J.pp2 = (const int32_t *)(in + o.s2.pp);
        J.pc1 = (const uint32_t *)(in + o.s1.pc); J.pc2 = (const uint32_t *)(in + o.s2.pc);
        J.pv1 = (const float *)(in + o.s1.pv); J.pv2 = (const float *)(in + o.s2.pv);
        J.pu1 = (const uint32_t *)(in + o.s1.pu); J.pu2 = (const uint32_t *)(in + o.s2.pu);
        J.g1f = (float *)(w + o.g1f); J.a1 = (float *)(w + o.a1);
        J.t2 = (float *)(w + o.t2); J.b2 = (float *)(w + o.aux2);
        J.map1 = (uint32_t *)(ob + o.map1); J.map2 = (uint32_t *)(ob + o.map2);
        J.mark_score = (float *)(w + o.ms); J.mark_prev = (uint32_t *)(w + o.mp);
        J.tb1 = (PgmTbNode *)(w + o.tb1); J.tb2 = (PgmTbNode *)(w + o.tb2);
        J.result = (PgmJob::Result *)(ob + o.res);
        J.hmap1 = (uint32_t *)(h_out_dev + o.map1); J.hmap2 = (uint32_t *)(h_out_dev + o.map2);
        J.hresult = (PgmJob::Result *)(h_out_dev + o.res);
        J.cells = (float4 *)(b->d_cells + o.cells);
        J.codes = (uint32_t *)(w + o.codes);
        J.endcell = (float4 *)(w + o.endcell);
        if (J.lean && !J.keep_cells && b->d_tabhdr) { J.cls1 = w + o.cls; J.cls2 = w + o.cls + J.n1; J.tabhdr = b->d_tabhdr + (size_t)PGM_TAB_HDR * i; }
        else { J.cls1 = nullptr; J.cls2 = nullptr; J.tabhdr = nullptr; }
        J.S = (float *)(b->d_S + o.S);
        J.prog = b->d_sync + o.prog;
        J.ltab = (uint16_t *)(w + o.ltab); J.lready = b->d_sync + o.lready; J.lrows = o.lrows; J.lcols = o.lcols;
        J.times = b->d_times + 2 * (size_t)i;
    }
}

// launch order: largest job first
static std::vector<uint32_t> size_order(const std::vector<PgmJob> &jobs) {
    std::vector<uint32_t> order(jobs.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return (uint64_t)jobs[x].n1 * jobs[x].n2 > (uint64_t)jobs[y].n1 * jobs[y].n2; });
    return order;
}
}  // namespace

extern "C" {

int pgm_test_cu_shares(uint32_t cus, double lean_cost, uint32_t nlean, double band_cost, uint32_t nbands, double rest_cost, uint32_t nrest,
                       uint32_t ncrit, double longest_chain, uint32_t *out4) {
    if (!out4) return fail(PGM_ERR_INVALID, "null argument");
    const CuShares r = cu_shares(cus, lean_cost, nlean, band_cost, nbands, rest_cost, nrest, ncrit, longest_chain);
    out4[0] = r.lean; out4[1] = r.band; out4[2] = r.crit; out4[3] = r.rest;
    return PGM_OK;
}

int pgm_test_batch_plan(uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2, const pgm_model *const *model,
                        const pgm_scores *scores, uint32_t flags, const pgm_site_ref *res1, const pgm_site_ref *res2, uint32_t cus,
                        uint32_t *head, double *dhead, uint32_t *job_fields, uint32_t *items, uint32_t *bands, uint32_t *lean_list, int32_t *tblist) {
    if (!head || !dhead || !items || !bands || (njobs && (!g1 || !g2 || !model || !scores || !job_fields || !lean_list || !tblist))) return fail(PGM_ERR_INVALID, "null argument");
    std::vector<char> two_chains(njobs, 0);
    for (uint32_t i = 0; i < njobs; ++i) two_chains[i] = job_is_two_chains(g1[i], g2[i]) ? 1 : 0;
    std::vector<PgmJob> jobs;
    BatchSizes Z;
    const int invalid = plan_sizes(njobs, g1, g2, model, scores, flags, res1, res2, two_chains, cus, jobs, Z);
    if (invalid >= 0) return fail(PGM_ERR_INVALID, "invalid job " + std::to_string(invalid));
    std::vector<uint8_t> image(std::max<size_t>(Z.in_base[njobs], 16));
    for (uint32_t i = 0; i < njobs; ++i)
        if (!plan_flatten_job(image.data(), Z.in_base[i], Z.in_base[i + 1], g1[i], g2[i], model[i], site_ref_of(res1, i), site_ref_of(res2, i), Z.pro, jobs[i], Z.off[i]))
            return fail(PGM_ERR_INVALID, "invalid graph in job " + std::to_string(i));
    const BatchSchedule S = plan_schedule(jobs, size_order(jobs), cus);
    const uint32_t h[PGM_PLAN_HEAD] = {njobs ? Z.pro.batch_dp : 0u, Z.pro.promote_bands, S.nitems, S.ncrit, S.nbands, S.nbands_narrow, S.nlean, S.ntb, S.ntb_c, S.ntb_b,
                                       S.nworkers, S.nlean_workers, S.nband_workers, S.nwide_workers, S.ncrit_workers, S.ntb_workers, S.ntb_b_workers,
                                       S.crit_c3, S.rest_c3, S.capacity, (uint32_t)S.total_b, (uint32_t)S.total, (uint32_t)S.total_c};
    const double d[PGM_PLAN_DHEAD] = {S.rsweep, S.t_goal, S.lean_cost, S.band_cost, S.band_end, S.other_cost, S.fill_end, S.crit_end, Z.pro.longest_crit_chain};
    memcpy(head, h, sizeof h);
    memcpy(dhead, d, sizeof d);
    for (uint32_t i = 0; i < njobs; ++i) {
        const PgmJob &J = jobs[i];
        const uint32_t f[PGM_PLAN_JOB] = {J.lean, J.has_extras, J.mode2, J.hD, J.hDX, J.slot_bytes, J.aux_off, J.ov_off, J.rh_off, J.c3_off, J.nov2, J.has_far, J.long1, J.long2,
                                          J.crit3, J.far_slack, J.nslots, Z.off[i].s1.ngeneric + Z.off[i].s2.ngeneric, Z.off[i].s1.nkill + Z.off[i].s2.nkill};
        memcpy(job_fields + (size_t)PGM_PLAN_JOB * i, f, sizeof f);
    }
    if (S.nitems) memcpy(items, S.items.data(), sizeof(PgmItem) * S.nitems);
    if (S.nbands) memcpy(bands, S.bands.data(), sizeof(PgmItem) * S.nbands);
    if (S.nlean) memcpy(lean_list, S.lean_list.data(), 4 * (size_t)S.nlean);
    if (S.ntb + S.ntb_c + S.ntb_b) memcpy(tblist, S.tblist.data(), 8 * (size_t)(S.ntb + S.ntb_c + S.ntb_b));
    return PGM_OK;
}

int pgm_align_batch_create(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                           const pgm_model *const *model, const pgm_scores *scores, pgm_align_batch **out) {
    return pgm_align_batch_create_ex(ctx, njobs, g1, g2, model, scores, 0u, out);
}

int pgm_align_batch_create_ex(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                              const pgm_model *const *model, const pgm_scores *scores, uint32_t flags, pgm_align_batch **out) {
    return pgm_align_batch_create_res(ctx, njobs, g1, g2, model, scores, flags, nullptr, nullptr, out);
}

int pgm_align_batch_create_res(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                               const pgm_model *const *model, const pgm_scores *scores, uint32_t flags,
                               const pgm_site_ref *res1, const pgm_site_ref *res2, pgm_align_batch **out) {
    if (!ctx || !out || (njobs && (!g1 || !g2 || !model || !scores))) return fail(PGM_ERR_INVALID, "null argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    const double tcs = now_ms();
    const bool cprof = getenv("PGM_HOST_PROFILE") != nullptr;   // tools: where the time of create goes
    const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
    BatchAlloc A;
    CreateGuard G{ctx, new pgm_align_batch, {}};
    pgm_align_batch *b = G.b;
    b->njobs = njobs;
    // ---- pass 1: validate and size.  (which jobs are two chains: a walk over both graphs' edges, on the host threads — 0.25 ms of a 128-job leaf level otherwise)
    std::vector<char> two_chains(njobs, 0);
    (void)lib_pool().run(njobs, njobs >= 16 ? 16u : 1u, [&](size_t i) { two_chains[i] = job_is_two_chains(g1[i], g2[i]) ? 1 : 0; });
    BatchSizes Z;
    const int invalid = plan_sizes(njobs, g1, g2, model, scores, flags, res1, res2, two_chains, cus, b->jobs, Z);
    if (invalid >= 0) return fail(PGM_ERR_INVALID, "invalid job " + std::to_string(invalid));
    const std::vector<size_t> &in_base = Z.in_base;
    b->maxdim = Z.maxdim; b->maxnb = Z.maxnb; b->maxn = Z.maxn; b->maxnblk = Z.maxnblk; b->cells = Z.cells;
    b->res_off.resize(njobs); b->map1_off.resize(njobs); b->map2_off.resize(njobs);
    for (uint32_t i = 0; i < njobs; ++i) { b->res_off[i] = Z.off[i].res; b->map1_off[i] = Z.off[i].map1; b->map2_off[i] = Z.off[i].map2; }
    b->in_bytes = std::max<size_t>(in_base[njobs], 16);
    b->work_bytes = std::max<size_t>(Z.L.W.bytes, 16);
    b->cell_bytes = std::max<size_t>(Z.L.C.bytes, 16);
    b->out_bytes = std::max<size_t>(Z.L.O.bytes, 16);
    b->s_bytes = std::max<size_t>(Z.L.SL.bytes, 16);
    b->lq_off = (uint32_t)Z.L.sync_ints;                   // ids of the jobs whose tracebacks have started (pre-link announcements)
    b->sync_ints = Z.L.sync_ints + 3 * (((size_t)njobs + 3) / 4 * 4);  // (one array per instance of pgm_tb_kernel)
    const double tc0 = now_ms();
    const SmallLayout sm = layout_small(b);
    // ---- the allocation thread; meanwhile pass 2 (the library's host threads): every job is flattened straight into a pinned staging
    // buffer (kept by the context) and its sweep planned
    G.alloc = std::thread(take_batch_buffers, ctx, b, sm, &A);
    hipError_t e;
    if ((e = cache_take(ctx, pgm_ctx::C_HIN, b->in_bytes, (void **)&b->h_in, &b->cap[pgm_ctx::C_HIN])) != hipSuccess)
        return fail(PGM_ERR_DEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    const double tc1 = now_ms();
    std::atomic<int> bad(-1), upload_err((int)hipSuccess);
    const uint32_t chunk_jobs = (uint32_t)std::max<size_t>(1, ((size_t)8 << 20) / std::max<size_t>(1, in_base[njobs] / std::max(1u, njobs)));
    std::vector<std::atomic<uint32_t>> chunk_done((njobs + chunk_jobs - 1) / chunk_jobs + 1);
    for (auto &cd : chunk_done) cd.store(0);
    (void)lib_pool().run(njobs, 16, [&](size_t job_index) {
        const uint32_t i = (uint32_t)job_index;
        if (!plan_flatten_job(b->h_in, in_base[i], in_base[i + 1], g1[i], g2[i], model[i], site_ref_of(res1, i), site_ref_of(res2, i), Z.pro, b->jobs[i], Z.off[i])) { bad.store((int)i); return; }
        // the input image goes to the device in chunks of consecutive jobs (~8 MB: a copy has ~10 us of fixed cost) while
        // the other jobs are still being flattened: whoever completes a chunk's last job sends it
        const uint32_t c = i / chunk_jobs, c0 = c * chunk_jobs, c1 = std::min(njobs, c0 + chunk_jobs);
        if (chunk_done[c].fetch_add(1, std::memory_order_acq_rel) + 1 == c1 - c0) {
            int st;
            while ((st = A.state.load(std::memory_order_acquire)) == 0) std::this_thread::yield();
            if (st == 1) {
                (void)hipSetDevice(ctx->device);
                const hipError_t eu = hipMemcpyAsync(b->d_in + in_base[c0], b->h_in + in_base[c0], in_base[c1] - in_base[c0], hipMemcpyHostToDevice, ctx->stream);
                if (eu != hipSuccess) upload_err.store((int)eu);
            }
        }
    });
    if (bad.load() >= 0) return fail(PGM_ERR_INVALID, "invalid graph in job " + std::to_string(bad.load()));
    const double tc2 = now_ms();
    G.alloc.join();
    const double tc3 = now_ms();
    if (A.err != hipSuccess) return fail(A.err == hipErrorOutOfMemory ? PGM_ERR_NOMEM : PGM_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(A.err));
    if (A.host_err != hipSuccess) return fail(PGM_ERR_DEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(A.host_err));
    // ---- device pointers, the schedule, the uploads
    bind_job_pointers(b, Z.off, res1, res2, A.h_out_dev);
    b->order = size_order(b->jobs);
    b->sched = plan_schedule(b->jobs, b->order, cus);
    const BatchSchedule &S = b->sched;
    if (cprof && njobs)
        fprintf(stderr, "    work lists: longest chain of sweeps %.0f us, goal %.0f us; lean %zu jobs %.0f us-worker on %u CUs; bands %zu, %.0f us-worker on %u CUs (simulated end %.0f us); items %zu, %.0f us-worker on %u CUs (simulated end %.0f us), of the longest chains %zu on %u CUs (%.0f us)\n",
                S.rsweep, S.t_goal, (size_t)S.nlean, S.lean_cost, S.nlean_workers, S.total_b, S.band_cost, S.nband_workers, S.band_end, S.total, S.other_cost, S.capacity, S.fill_end, S.total_c, S.ncrit_workers, S.crit_end);
    const double tc4 = now_ms();
    if (S.nitems > std::max<size_t>(1, sm.total_bands)) return fail(PGM_ERR_DEVICE, "work list longer than the number of bands");   // (cannot happen: an item holds at least one band)
    if ((e = (hipError_t)upload_err.load()) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_tblist, S.tblist.data(), 8 * S.tblist.size(), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_jobs, b->jobs.data(), sizeof(PgmJob) * njobs, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_order, b->order.data(), 4 * (size_t)njobs, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_items, S.items.data(), sizeof(PgmItem) * S.items.size(), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_lean, S.lean_list.data(), 4 * S.lean_list.size(), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(b->d_bands, S.bands.data(), sizeof(PgmItem) * S.bands.size(), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
        (e = classify_lean_jobs(ctx, b)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        return fail(PGM_ERR_DEVICE, std::string("upload: ") + hipGetErrorString(e));
    // ---- events
    for (int k = 0; k < 5; ++k) (void)hipEventCreate(&b->ev[k]);
    (void)hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&b->ev_join_b, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&b->ev_join_c, hipEventDisableTiming);
    if (cprof)
        fprintf(stderr, "    create: sizes %.2f ms, pinned input block %.2f, flatten %.2f, wait for the allocations %.2f (device %.2f, pinned results %.2f), work list %.2f, upload of %.1f MB %.2f\n",
                tc0 - tcs, tc1 - tc0, tc2 - tc1, tc3 - tc2, A.ms_dev, A.ms_host, tc4 - tc3, b->in_bytes / 1e6, now_ms() - tc4);
    if (cprof)
        fprintf(stderr, "    device buffers: inputs %.1f MB %.2f ms, work %.1f MB %.2f, cells %.1f MB %.2f, results %.1f MB %.2f, S %.1f MB %.2f, small %.2f\n",
                b->in_bytes / 1e6, A.ms_slot[0], b->work_bytes / 1e6, A.ms_slot[1], b->cell_bytes / 1e6, A.ms_slot[2], b->out_bytes / 1e6, A.ms_slot[3], b->s_bytes / 1e6, A.ms_slot[4], A.ms_slot[5]);
    *out = G.release();
    return PGM_OK;
}

int pgm_align_batch_run(pgm_ctx *ctx, pgm_align_batch *b) {
    if (!ctx || !b) return fail(PGM_ERR_INVALID, "null argument");
    if (b->njobs == 0) return PGM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_all(ctx, b, true));   // (stage events: four event records per launch, read by fetch once the stream has completed)
    b->ev_pending = true;
    return PGM_OK;
}

int pgm_align_batch_time(pgm_ctx *ctx, pgm_align_batch *b, int reps, float *ms_prep, float *ms_emission, float *ms_fill,
                         float *ms_traceback) {
    if (!ctx || !b || reps <= 0) return fail(PGM_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    double acc[4] = {0, 0, 0, 0};
    for (int r = 0; r < reps && b->njobs; ++r) {
        HIPCHK(launch_all(ctx, b, true));
        b->ev_pending = false;
        HIPCHK(hipEventSynchronize(b->ev[4]));
        for (int k = 0; k < 4; ++k) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, b->ev[k], b->ev[k + 1]));
            acc[k] += ms;
        }
    }
    if (ms_prep) *ms_prep = (float)(acc[0] / reps);
    if (ms_emission) *ms_emission = (float)(acc[1] / reps);
    if (ms_fill) *ms_fill = (float)(acc[2] / reps);
    if (ms_traceback) *ms_traceback = (float)(acc[3] / reps);
    return PGM_OK;
}

int pgm_align_batch_job_times(pgm_ctx *ctx, pgm_align_batch *b, uint64_t *ticks) {
    if (!ctx || !b || !ticks) return fail(PGM_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (b->njobs) HIPCHK(hipMemcpy(ticks, b->d_times, 16 * (size_t)b->njobs, hipMemcpyDeviceToHost));
    return PGM_OK;
}

int pgm_align_batch_fetch(pgm_ctx *ctx, pgm_align_batch *b, pgm_align_out *out) {
    if (!ctx || !b || (b->njobs && !out)) return fail(PGM_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    if (b->njobs == 0) { HIPCHK(hipStreamSynchronize(ctx->stream)); return PGM_OK; }
    // results + mappings were written into the pinned block by the kernel itself (PgmJob::hmap1/hmap2/hresult): wait for
    // the stream, then scatter
    int rc = PGM_OK;
    HIPCHK(hipMemcpyAsync(b->h_flag, b->d_sync, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    // Finished jobs are copied out while the kernel is still running: a job's traceback worker writes the reversed mappings
    // and then the result record (status word last) into the pinned block; all but the largest jobs are done long before the
    // batch is, so only a few records are left when the stream completes.
    std::vector<uint8_t> copied(b->njobs, 0);
    auto collect = [&]() -> int {
        uint32_t n = 0;
        for (uint32_t i = 0; i < b->njobs; ++i) {
            if (copied[i]) { ++n; continue; }
            const PgmJob::Result *hr = (const PgmJob::Result *)(b->h_out + b->res_off[i]);
            const int32_t st = __atomic_load_n(&hr->status, __ATOMIC_ACQUIRE);
            if (st == PGM_STATUS_PENDING) continue;
            if (!out[i].map1 || !out[i].map2) return -1;
            const uint32_t len = hr->len;
            if (len > b->jobs[i].n1 + b->jobs[i].n2) return -2;
            out[i].score = hr->score; out[i].n_tr_indels = hr->n_tr_indels; out[i].len = len; out[i].status = st;
            memcpy(out[i].map1, b->h_out + b->map1_off[i], 4 * (size_t)len);
            memcpy(out[i].map2, b->h_out + b->map2_off[i], 4 * (size_t)len);
            copied[i] = 1; ++n;
        }
        return (int)n;
    };
    for (;;) {
        const int n = collect();
        if (n < 0) { (void)hipStreamSynchronize(ctx->stream); return fail(n == -1 ? PGM_ERR_INVALID : PGM_ERR_DEVICE, n == -1 ? "null mapping buffer" : "corrupt result length"); }
        if ((uint32_t)n == b->njobs) break;
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipSuccess) break;                       // (an aborted launch leaves records pending)
        if (q != hipErrorNotReady) return fail(PGM_ERR_DEVICE, std::string("fill kernel: ") + hipGetErrorString(q));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (b->ev_pending) {   // stage times of the launch just completed (pgm_align_batch_stage_times)
        b->ev_pending = false;
        float ms[3] = {0, 0, 0};
        bool ok = true;
        for (int k = 0; k < 3; ++k) ok = ok && hipEventElapsedTime(&ms[k], b->ev[k], b->ev[k + 1]) == hipSuccess;
        if (ok) { for (int k = 0; k < 3; ++k) b->acc_ms[k] += ms[k]; ++b->acc_n; }
        else (void)hipGetLastError();
    }
    const int aborted = *b->h_flag;
    if (aborted) return fail(PGM_ERR_DEVICE, "fill kernel: a band hand-off timed out");
    for (uint32_t i = 0; i < b->njobs; ++i) {
        PgmJob::Result res;
        memcpy(&res, b->h_out + b->res_off[i], sizeof res);
        if (res.status == PGM_STATUS_PENDING) return fail(PGM_ERR_DEVICE, "fill kernel: a job's result record was never written");
        if (res.status != PGM_OK) rc = res.status;
        if (copied[i]) continue;
        out[i].score = res.score;
        out[i].n_tr_indels = res.n_tr_indels;
        out[i].len = res.len;
        out[i].status = res.status;
        if (res.status != PGM_OK) rc = res.status;
        if (!out[i].map1 || !out[i].map2) return fail(PGM_ERR_INVALID, "null mapping buffer");
        if (res.len > b->jobs[i].n1 + b->jobs[i].n2) return fail(PGM_ERR_DEVICE, "corrupt result length");
        memcpy(out[i].map1, b->h_out + b->map1_off[i], 4 * (size_t)res.len);
        memcpy(out[i].map2, b->h_out + b->map2_off[i], 4 * (size_t)res.len);
    }
    if (rc != PGM_OK) g_err = "backtracking failed";
    return rc;
}

void pgm_align_batch_destroy(pgm_ctx *ctx, pgm_align_batch *b) {
    if (!b) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }   // nothing of the batch is in flight when its buffers go back to the cache
    if (ctx && ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx && ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    if (ctx && ctx->stream4) (void)hipStreamSynchronize(ctx->stream4);
    for (int k = 0; k < 5; ++k)
        if (b->ev[k]) (void)hipEventDestroy(b->ev[k]);
    if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
    if (b->ev_join) (void)hipEventDestroy(b->ev_join);
    if (b->ev_join_b) (void)hipEventDestroy(b->ev_join_b);
    if (b->ev_join_c) (void)hipEventDestroy(b->ev_join_c);
    for (const BatchBuffer &e : kBatchBuffers) cache_give(ctx, e.slot, b->*e.ptr, b->cap[e.slot]);
    cache_give(ctx, pgm_ctx::C_HOST, b->h_out, b->cap[pgm_ctx::C_HOST]);
    cache_give(ctx, pgm_ctx::C_HIN, b->h_in, b->cap[pgm_ctx::C_HIN]);
    delete b;
}

uint64_t pgm_align_batch_cells(const pgm_align_batch *b) { return b ? b->cells : 0; }

int pgm_align_batch_stage_times(pgm_align_batch *b, int reset, float *ms_prep, float *ms_emission, float *ms_fill, uint32_t *launches) {
    if (!b) return fail(PGM_ERR_INVALID, "null batch");
    const double n = b->acc_n ? (double)b->acc_n : 1.0;
    if (ms_prep) *ms_prep = (float)(b->acc_ms[0] / n);
    if (ms_emission) *ms_emission = (float)(b->acc_ms[1] / n);
    if (ms_fill) *ms_fill = (float)(b->acc_ms[2] / n);
    if (launches) *launches = b->acc_n;
    if (reset) { b->acc_ms[0] = b->acc_ms[1] = b->acc_ms[2] = 0; b->acc_n = 0; }
    return PGM_OK;
}

int pgm_align_batch_test_stall(pgm_align_batch *b, uint32_t job, uint32_t band, uint32_t spin_limit) {
    if (!b) return fail(PGM_ERR_INVALID, "null batch");
    b->test_stall_job = job; b->test_stall_band = band; b->test_spin_limit = spin_limit;
    return PGM_OK;
}

int pgm_align_graphs_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                           const pgm_model *const *model, const pgm_scores *scores, pgm_align_out *out) {
    return pgm_align_graphs_batch_res(ctx, njobs, g1, g2, model, scores, nullptr, nullptr, out);
}

int pgm_align_graphs_batch_res(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                               const pgm_model *const *model, const pgm_scores *scores, const pgm_site_ref *res1, const pgm_site_ref *res2,
                               pgm_align_out *out) {
    pgm_align_batch *b = nullptr;
    const bool prof = getenv("PGM_HOST_PROFILE") != nullptr;   // tools: where the time of one call goes
    const auto t0 = std::chrono::steady_clock::now();
    int rc = pgm_align_batch_create_res(ctx, njobs, g1, g2, model, scores, 0u, res1, res2, &b);
    if (rc != PGM_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    {
        // One stage of persistent grids per DEVICE at a time: every batch sizes its grids for the whole device (no grid of a stage waits
        // for a CU, see pgm_tb_kernel's header), so two contexts on one device take turns here.  (Callers of the create / run / fetch
        // interface with several contexts on a device have to do the same.)
        static std::mutex device_turn[64];
        std::lock_guard<std::mutex> turn(device_turn[(unsigned)ctx->device % 64u]);
        rc = pgm_align_batch_run(ctx, b);
        if (rc == PGM_OK) rc = pgm_align_batch_fetch(ctx, b, out);
    }
    const auto t2 = std::chrono::steady_clock::now();
    pgm_align_batch_destroy(ctx, b);
    if (prof)
        fprintf(stderr, "  pgm_align_graphs_batch: %u jobs, create (flatten, allocate, upload, work list) %.2f ms, run + fetch %.2f ms, destroy %.2f ms\n", njobs,
                std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
    return rc;
}

int pgm_align_batch_read_matrices(pgm_ctx *ctx, pgm_align_batch *b, uint32_t job, float *M, float *X, float *Y, float *W, float *S) {
    if (!ctx || !b || job >= b->njobs) return fail(PGM_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const PgmJob &J = b->jobs[job];
    const size_t N = (size_t)J.n1 * J.n2;
    if ((M || X || Y || W) && !J.keep_cells)
        return fail(PGM_ERR_INVALID, "the DP matrices of a chain-only job are only kept for a batch created with PGM_BATCH_KEEP_MATRICES");
    if (S && J.tabhdr) {   // (a job of two sequence graphs looks its scores up in a class table: nothing was written to S)
        int bad = 1;
        HIPCHK(hipMemcpy(&bad, J.tabhdr, sizeof(int), hipMemcpyDeviceToHost));
        if (bad == 0) return fail(PGM_ERR_INVALID, "the score matrix of a job of two sequence graphs is only stored for a batch created with PGM_BATCH_KEEP_MATRICES");
    }
    if (M || X || Y || W) {
        const uint32_t sh = J.rshift, R = 1u << sh;
        const size_t ncell = (size_t)J.nb * J.tsteps * 64u * R;
        std::vector<float4> cells(ncell);
        HIPCHK(hipMemcpy(cells.data(), J.cells, ncell * sizeof(float4), hipMemcpyDeviceToHost));
        float *dst[4] = {M, X, Y, W};
        for (int k = 0; k < 4; ++k)
            if (dst[k]) std::fill(dst[k], dst[k] + N, -INFINITY);
        for (uint32_t y = 0; y + 1 < J.n1; ++y)
            for (uint32_t x = 0; x < J.ncol; ++x) {
                const uint32_t bb = y >> (6u + sh), w = y & ((64u << sh) - 1u), l = w >> sh, r = w & (R - 1u);
                const float4 c = cells[((((size_t)bb * J.tsteps + (x + l)) << sh) | r) * 64u + l];  // {M, X, W, Y}
                const size_t i = (size_t)y + (size_t)J.n1 * x;
                if (M) M[i] = c.x;
                if (X) X[i] = c.y;
                if (Y) Y[i] = c.w;
                if (W) W[i] = c.z;
            }
    }
    if (S) {
        // the emission scores exactly as the fill kernel consumes them (PgmJob::S, written by pgm_emission_skew_kernel), de-skewed
        const uint32_t sh = J.rshift, R = 1u << sh;
        const size_t ns = (size_t)J.nb * J.nblk * 64u * PGM_BLOCK * R;
        std::vector<float> sk(ns);
        HIPCHK(hipMemcpy(sk.data(), J.S, ns * sizeof(float), hipMemcpyDeviceToHost));
        std::fill(S, S + N, 0.0f);
        for (uint32_t y = 0; y + 1 < J.n1; ++y)
            for (uint32_t x = 0; x < J.ncol; ++x) {
                const uint32_t bb = y >> (6u + sh), w = y & ((64u << sh) - 1u), l = w >> sh, r = w & (R - 1u), t = x + l;
                S[(size_t)y + (size_t)J.n1 * x] = sk[(((((size_t)bb * J.nblk + t / PGM_BLOCK) << sh) | r) * 64u + l) * PGM_BLOCK + t % PGM_BLOCK];
            }
    }
    return PGM_OK;
}

}  // extern "C"

#include "pgm_nw_capi.inc"
#include "pgm_csprofile_capi.inc"
#include "pgm_dist_capi.inc"
#include "pgm_merge_capi.inc"
#include "pgm_parsimony_capi.inc"
#include "pgm_wls_capi.inc"
#include "pgm_bionj_capi.inc"
#include "pgm_agreement_capi.inc"
#include "pgm_transfer_capi.inc"
#include "pgm_transfer_taxa_capi.inc"
#include "pgm_treelik_capi.inc"
#include "pgm_resample_capi.inc"
