// pgm_plan.h — the host-only planning of an align batch: flattening of the graphs, the sweep each job gets and the LDS layout of
// its sweeping wavefront (plan_job_sweep), the work lists, their order and the CUs of every launch (plan_schedule).  Pure
// arithmetic on graph sizes and edge summaries: no kernel header, no HIP runtime call (compiles with a plain host compiler).
// pgm_align_batch_create_res (pgm_capi.hip) and the test hook pgm_test_batch_plan go through the same functions.
#ifndef PGM_PLAN_H_
#define PGM_PLAN_H_

#include <hip/hip_vector_types.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <queue>
#include <vector>

#include "pgm_device.h"

namespace {

// ---- step times (us per step, measured with the whole batch resident), lags and thresholds of the planning -------------
constexpr double kTauChain = 0.45;    // a chain-only band (the leaf level is bound by the HBM write bandwidth)
constexpr double kTauExtras = 0.65;   // ... with the near window and the far history in the sweeping wavefront
constexpr double kTauMode2 = 0.6;     // ... with helpers
constexpr double kTauCrit = 0.42;     // a band of a crit3 job (pgm_crit_kernel); also what a batch swept as MODE 2, one band per CU, is estimated with
constexpr double kTauLean = 0.34;     // lean sweep: us per step of R rows per lane
constexpr double kEager = 0.7;        // items with a remaining path above this share of the longest get a worker at once
constexpr double kLag = PGM_ROWS + 3.0 * PGM_BLOCK;   // band-to-band lag of the work lists (steps): 88
constexpr double kLagCritEst = 80.0;  // ... of the chain the batch's largest job would have in pgm_crit_kernel (from the sizes alone)
constexpr double kLagWideEst = 78.0;  // ... of a job's chain of self-contained sweeps on a WIDE worker
constexpr uint32_t kNarrowSlot = PGM_POOL / PGM_WAVES / 16 * 16;        // a sweep that fits an eighth of a CU's LDS
constexpr uint32_t kWideSlot = PGM_POOL / PGM_WIDE_WAVES / 16 * 16;     // ... a quarter
// (a job with helper wavefronts: one of at least kMode2MinBands bands, or one whose history of at least kMode2MinHd steps does not fit WIDE)
constexpr uint32_t kMode2MinBands = 20u, kMode2MinHd = 32u;
constexpr uint32_t kC3Bytes = 4096 + 6 * 2048;   // extra LDS of a crit3 sweep (PGM_C3_BYTES of pgm_crit_kernels.h; pgm_capi.hip asserts they agree)
constexpr uint32_t kOvBytes = 8u * PGM_OV_REC * PGM_OV_ENT;   // the overflow table's copy in LDS
// bands of 64 rows of a graph with n nodes (one row per lane, whatever the job's rshift)
inline uint32_t row_bands(uint32_t n) { return (n - 1 + PGM_ROWS - 1) / PGM_ROWS; }
// the alphabet tier of a batch: 4 (nucleotides: a node's profile is one float4), 20 (amino acids), 64 (codons)
inline uint32_t alphabet_tier(uint32_t dim) { return dim <= 4 ? 4u : dim <= 20 ? 20u : 64u; }

// ---- arena: one host staging buffer mirrored by one device allocation ------------------------
struct Arena {   // bump allocator over a slice [off, end) of an external host buffer; offsets are relative to `base`
    uint8_t *base = nullptr;
    size_t off = 0, end = 0;
    bool overflow = false;
    size_t put(const void *src, size_t bytes, size_t align = 16) {
        const size_t o = (off + align - 1) / align * align;
        if (o + bytes > end) { overflow = true; return 0; }
        off = o + bytes;
        if (src && bytes) memcpy(base + o, src, bytes);
        return o;
    }
};
struct DevLayout {  // sizes of device-only regions
    size_t bytes = 0;
    size_t take(size_t b, size_t align = 256) {
        size_t off = (bytes + align - 1) / align * align;
        bytes = off + b;
        return off;
    }
};

// ---- flattening of one graph side -------------------------------------------------------------
struct SideOff {
    size_t sites, ni, xp, xc, xv, pp, pc, pv, pu, fp, fe, ov;
    size_t smap = 0;              // resident profiles: the node -> column map of the side
    bool has_smap = false;
    uint32_t nodes_with_extras;   // nodes with a predecessor other than the chain neighbour
    uint32_t has_long;            // some edge outside the near slots is longer than PGM_DCAP
    uint32_t maxd_cap;            // largest distance <= PGM_DCAP of an edge outside the chain slot (>= 1)
    uint32_t maxd_kf8;            // ... among the nodes with at most PGM_KF8 far candidates, none of them long
    // set by finalize_side, once the job's sweep mode is known:
    uint32_t far_nodes;           // nodes with entries served from the LDS history
    uint32_t maxd;                // largest on-chip predecessor distance of the graph (>= 1)
    uint32_t far_dmin;            // smallest distance of a far entry (PGM_DCAP + 1 if there is none)
    uint32_t remote;              // MODE 2: entries served from the cell storage by the far helpers
    uint32_t nov;                 // MODE 2, columns: records of the overflow table in use
    uint32_t ngeneric;            // nodes served by the generic path
    uint32_t nkill;               // interior nodes without predecessors
    // host only: far candidates (every finite edge outside the near slots) of node v: [cp[v], cp[v+1])
    std::vector<uint32_t> cp, cd;
    std::vector<float> cv;
};

static int flatten_side(const pgm_graph *g, const pgm_scores &sc, Arena &A, SideOff &o, const pgm_site_ref *res = nullptr) {
    const uint32_t n = g->n;
    const bool resident = res && res->dev_sites;
    if (n < 2 || (!g->sites && !resident) || !g->e_rowptr) return PGM_ERR_INVALID;
    // (scratch of the calling pool thread, kept between jobs: sixteen threads allocating and freeing ~150 KB per side
    // contend for the address space with the allocation thread's hipMalloc)
    static thread_local std::vector<float> xv, pv;
    static thread_local std::vector<int32_t> xp, pp;
    static thread_local std::vector<uint32_t> xc, pc, pu;
    static thread_local std::vector<PgmNode2> ni;
    xv.clear(); pv.clear(); xc.clear(); pc.clear(); pu.clear();
    xp.assign(n + 1, 0); pp.assign(n + 1, 0);
    ni.resize(n);
    o.nodes_with_extras = 0; o.has_long = 0; o.maxd_cap = 1; o.maxd_kf8 = 1; o.nkill = 0;
    o.cp.assign(n + 1, 0); o.cd.clear(); o.cv.clear();
    for (uint32_t v = 0; v < n; ++v) {
        PgmNode2 &I = ni[v];
        memset(&I, 0, sizeof I);
        I.cc = I.c2 = I.c3 = INFINITY;
        for (int k = 0; k < PGM_KF8; ++k) I.fc[k] = INFINITY;
        // near slots: the first finite-cost edge from node-1 / node-2 / node-3; everything else is a far candidate (an edge
        // of infinite cost contributes -inf to every maximum: it only stays in the CSR lists)
        auto place = [&](uint32_t from, float val) {
            const uint32_t d = v - from;
            if (d == 1 && I.cc == INFINITY && val != INFINITY) { I.cc = val; return; }
            xc.push_back(from); xv.push_back(val);
            if (val == INFINITY) return;
            if (d <= (uint32_t)PGM_DCAP) o.maxd_cap = std::max(o.maxd_cap, d); else o.has_long = 1;
            if (d == 2 && I.c2 == INFINITY) { I.c2 = val; return; }
            if (d == 3 && I.c3 == INFINITY) { I.c3 = val; return; }
            o.cd.push_back(d); o.cv.push_back(val);
        };
        const int32_t eb = g->e_rowptr[v], ee = g->e_rowptr[v + 1];
        if (eb > ee || eb < 0) return PGM_ERR_INVALID;
        for (int32_t e = eb; e < ee; ++e) {
            const uint32_t from = g->e_col[e];
            if (from >= v) return PGM_ERR_INVALID;  // edges must point to earlier nodes (Graph.h:43, GraphAlign.h:631-656)
            const float c = g->e_val[e];
            const float val = (c == 0) ? INFINITY : c + 10000.0f;  // PredIterator::value, Graph.h:223-231
            pc.push_back(from); pv.push_back(val); pu.push_back(0u);
            place(from, val);
        }
        if (g->r_rowptr) {
            if (g->r_rowptr[v] > g->r_rowptr[v + 1] || g->r_rowptr[v] < 0) return PGM_ERR_INVALID;
            for (int32_t e = g->r_rowptr[v]; e < g->r_rowptr[v + 1]; ++e) {
                const uint32_t from = g->r_col[e];
                if (from >= v) return PGM_ERR_INVALID;
                const uint32_t units = g->r_units[e];
                const float val = (units == 0) ? INFINITY : sc.repeat_init + sc.repeat_ext * (float)(units - 1);  // Graph.h:232-238
                pc.push_back(from); pv.push_back(val); pu.push_back(0x80000000u | units);
                place(from, val);
            }
        }
        xp[v + 1] = (int32_t)xc.size();
        pp[v + 1] = (int32_t)pc.size();
        o.cp[v + 1] = (uint32_t)o.cd.size();
        {
            uint32_t dm = I.c3 != INFINITY ? 3u : (I.c2 != INFINITY ? 2u : 1u);
            bool small = o.cp[v + 1] - o.cp[v] <= (uint32_t)PGM_KF8;
            for (uint32_t k = o.cp[v]; k < o.cp[v + 1] && small; ++k) { if (o.cd[k] > (uint32_t)PGM_DCAP) small = false; else dm = std::max(dm, o.cd[k]); }
            if (small) o.maxd_kf8 = std::max(o.maxd_kf8, dm);
        }
        if (v > 0 && v + 1 < n && pp[v + 1] == pp[v]) { I.flags |= PGM_NF_KILL; ++o.nkill; }  // interior node without predecessors
        o.nodes_with_extras += (xp[v + 1] > xp[v]);
    }
    // at least one element each so that pointers are valid
    if (xc.empty()) { xc.push_back(0); xv.push_back(0); }
    if (pc.empty()) { pc.push_back(0); pv.push_back(0); pu.push_back(0); }
    o.smap = 0; o.has_smap = false;
    if (resident) {   // the profiles are in HBM already (pgm_merge_profiles_batch_ex): only the node -> column map travels
        // (the prep kernel gathers column node_map[v] of the device matrix unchecked: the range is checked here)
        if (res->ncols == 0 || (!res->node_map && n > res->ncols)) return PGM_ERR_INVALID;
        if (res->node_map) for (uint32_t v = 0; v < n; ++v) if (res->node_map[v] >= res->ncols) return PGM_ERR_INVALID;
        o.sites = 0;
        if (res->node_map) { o.smap = A.put(res->node_map, 4 * (size_t)n); o.has_smap = true; }
    } else o.sites = A.put(g->sites, sizeof(double) * (size_t)g->dim * n);
    o.ni = A.put(ni.data(), sizeof(PgmNode2) * ni.size());
    o.xp = A.put(xp.data(), 4 * xp.size());
    o.xc = A.put(xc.data(), 4 * xc.size());
    o.xv = A.put(xv.data(), 4 * xv.size());
    o.pp = A.put(pp.data(), 4 * pp.size());
    o.pc = A.put(pc.data(), 4 * pc.size());
    o.pv = A.put(pv.data(), 4 * pv.size());
    o.pu = A.put(pu.data(), 4 * pu.size());
    o.fp = A.put(nullptr, 4 * ((size_t)n + 1));                             // filled by finalize_side
    o.fe = A.put(nullptr, 8 * std::max<size_t>(1, o.cd.size()));
    o.ov = A.put(nullptr, 8 * (size_t)PGM_OV_REC * PGM_OV_ENT);
    return PGM_OK;
}

// Second half of the flattening, once the sweep mode of the job is known: where the far candidates of every node go.
//   self-contained sweep (MODE 1): up to PGM_KF entries of distance <= PGM_DCAP in the node summary, else the node is generic
//   MODE 2, rows (side 0): every candidate into the row CSR fp / fe, remote if farther than PGM_DCAP or above the virtual
//           lanes of the row's band; at most PGM_REMOTE_MAX remote and 512 entries per band (rows beyond that: generic)
//   MODE 2, columns (side 1): up to PGM_KF8 entries in the node summary, at most one of them LONG (slot 7)
static void finalize_side(uint8_t *base, uint32_t n, SideOff &o, int side, bool mode2, bool allow_long, bool allow_ov) {
    PgmNode2 *ni = (PgmNode2 *)(base + o.ni);
    int32_t *fp = (int32_t *)(base + o.fp);
    uint2 *fe = (uint2 *)(base + o.fe), *ov = (uint2 *)(base + o.ov);
    o.nov = 0;
    o.far_nodes = 0; o.maxd = 1; o.far_dmin = PGM_DCAP + 1; o.remote = 0; o.ngeneric = 0;
    uint32_t band_entries = 0, band_remote = 0, nfe = 0;
    fp[0] = 0;
    for (uint32_t v = 0; v < n; ++v) {
        PgmNode2 &I = ni[v];
        const uint32_t kill = I.flags & PGM_NF_KILL;
        const uint32_t c0 = o.cp[v], c1 = o.cp[v + 1], nc = c1 - c0;
        if (side == 0 && (v & 63u) == 0) { band_entries = 0; band_remote = 0; }
        uint32_t dmax = 1, nloc = 0, nrem = 0, novf = 0, ovi = 0;
        if (I.c2 != INFINITY) dmax = 2;
        if (I.c3 != INFINITY) dmax = 3;
        bool generic = false;
        if (!mode2) {
            if (nc > (uint32_t)PGM_KF) generic = true;
            for (uint32_t k = c0; k < c1 && !generic; ++k) {
                if (o.cd[k] > (uint32_t)PGM_DCAP) { generic = true; break; }
                I.fd[nloc] = o.cd[k]; I.fc[nloc] = o.cv[k]; ++nloc;
                dmax = std::max(dmax, o.cd[k]);
                o.far_dmin = std::min(o.far_dmin, o.cd[k]);
            }
        } else if (side == 0) {
            const uint32_t lane = v & 63u;
            for (uint32_t k = c0; k < c1; ++k) nrem += (o.cd[k] > (uint32_t)PGM_DCAP || o.cd[k] > lane + (uint32_t)PGM_VL);
            if (band_entries + nc > 512u || band_remote + nrem > (uint32_t)PGM_REMOTE_MAX || nc > 255u || (nrem && !allow_long)) generic = true;
            else {
                for (uint32_t k = c0; k < c1; ++k) {
                    const uint32_t d = o.cd[k];
                    const bool rem = d > (uint32_t)PGM_DCAP || d > lane + (uint32_t)PGM_VL;
                    fe[nfe++] = make_uint2(d | (rem ? 0x80000000u : 0u), __builtin_bit_cast(uint32_t, o.cv[k]));
                    if (!rem) { dmax = std::max(dmax, d); o.far_dmin = std::min(o.far_dmin, d); ++nloc; }
                }
                band_entries += nc; band_remote += nrem;
            }
        } else {
            for (uint32_t k = c0; k < c1; ++k) nrem += o.cd[k] > (uint32_t)PGM_DCAP;
            const uint32_t nl_all = nc - nrem, ring_cap = (uint32_t)PGM_KF8 - std::min(nrem, (uint32_t)PGM_KF8);
            novf = nl_all > ring_cap ? nl_all - ring_cap : 0u;
            if (nrem > (uint32_t)PGM_NLONG || (nrem && !allow_long) || novf > (uint32_t)PGM_OV_ENT || (novf && (o.nov >= (uint32_t)PGM_OV_REC || !allow_ov))) generic = true;
            else {
                uint2 *rec = ov + (size_t)o.nov * PGM_OV_ENT;
                uint32_t nl = 0, no = 0;
                for (uint32_t k = c0; k < c1; ++k) {
                    const uint32_t d = o.cd[k];
                    if (d > (uint32_t)PGM_DCAP) { I.fd[PGM_KF8 - 1 - nl] = d; I.fc[PGM_KF8 - 1 - nl] = o.cv[k]; ++nl; continue; }
                    if (nloc < ring_cap) { I.fd[nloc] = d; I.fc[nloc] = o.cv[k]; ++nloc; }
                    else rec[no++] = make_uint2(d, __builtin_bit_cast(uint32_t, o.cv[k]));
                    dmax = std::max(dmax, d); o.far_dmin = std::min(o.far_dmin, d);
                }
                if (novf) { ovi = o.nov++; for (; no < (uint32_t)PGM_OV_ENT; ++no) rec[no] = make_uint2(1u, __builtin_bit_cast(uint32_t, (float)INFINITY)); }
            }
        }
        fp[v + 1] = (int32_t)nfe;
        if (generic) {   // every non-chain predecessor of this node goes through the CSR lists and the cell storage
            I.c2 = I.c3 = INFINITY;
            for (int k = 0; k < PGM_KF8; ++k) { I.fd[k] = 0; I.fc[k] = INFINITY; }
            I.flags = PGM_NF_GENERIC | (1u << 8) | kill;
            ++o.ngeneric;
        } else {
            const bool rows2 = mode2 && side == 0;
            I.flags = (rows2 ? 0u : nloc) | (dmax << 8) | kill | ((mode2 && side == 1) ? (nrem << 16) | (novf << 20) | (ovi << 25) : 0u);
            o.maxd = std::max(o.maxd, dmax);
            o.far_nodes += (nloc + nrem) != 0;
            o.remote += nrem;
        }
    }
}

// Device-only regions of one job (offsets inside the batch's work / cell / result / score buffers) and its slice of the
// progress counters (pass 1 of pgm_align_batch_create).
struct JobOff { SideOff s1, s2; size_t M, pi, g1f, a1, t2, aux2, map1, map2, ms, mp, res, cells, tb1, tb2, S, prog, codes, endcell, ltab, lready, cls; uint32_t lrows, lcols; };
struct BatchLayout { DevLayout W, C, O, SL; size_t sync_ints = 64; };   // sync: [0] abort flag, [1] ticket counter of the band list, [2] of the lean list; on a cache line of their own, [32] pre-link tasks announced, [33] tracebacks finished (polled by every idle worker)
// dp: the padded stride of the converted profiles (PgmJob::dp), the same for every job of a batch
static void layout_job(BatchLayout &L, uint32_t n1, uint32_t n2, uint32_t dp, uint32_t rshift, bool lean, bool keep, JobOff &o) {
    const uint32_t R = 1u << rshift, rows = PGM_ROWS * R;
    const uint32_t nb = (n1 - 1 + rows - 1) / rows, tsteps = (n2 - 1) + 63;
    const uint32_t nblk = (tsteps + PGM_BLOCK - 1) / PGM_BLOCK, maxn = std::max(n1, n2);
    o.g1f = L.W.take(sizeof(float) * (size_t)dp * n1);
    o.a1 = L.W.take(sizeof(float) * n1);
    o.t2 = L.W.take(sizeof(float) * (size_t)dp * n2);
    o.aux2 = L.W.take(sizeof(float) * (size_t)n2);
    o.map1 = L.O.take(4 * (size_t)(n1 + n2), 16);
    o.map2 = L.O.take(4 * (size_t)(n1 + n2), 16);
    o.tb1 = L.W.take(sizeof(PgmTbNode) * (size_t)n1);
    o.tb2 = L.W.take(sizeof(PgmTbNode) * (size_t)n2);
    o.ms = L.W.take(4 * (size_t)maxn);
    o.mp = L.W.take(4 * (size_t)maxn);
    o.res = L.O.take(sizeof(PgmJob::Result), 16);
    o.cells = L.C.take(keep ? sizeof(float4) * (size_t)nb * tsteps * 64u * R : 16, 1024);   // (a lean job without the test hook: codes only)
    o.codes = L.W.take(lean ? 4 * (size_t)nb * nblk * 64u * R : 16);   // one word per lane, row and block of eight steps
    o.endcell = L.W.take(16, 16);
    o.cls = L.W.take((lean && !keep) ? (size_t)n1 + n2 : 16, 16);   // classes of the nodes of a lean job (PgmJob::cls1 / cls2)
    o.S = L.SL.take(sizeof(float) * (size_t)nb * nblk * 64u * PGM_BLOCK * R, 1024);
    o.prog = L.sync_ints;
    L.sync_ints += (nb + 3) / 4 * 4;
    // pre-linked traceback tiles (PgmJob::ltab): the long jobs of the general path (from PGM_LK_MIN_ROWS rows: the ones whose
    // tracebacks end a batch; pre-linking every job of the headline batch — 26 000 tiles — cost the sweeps still running 30 %)
    o.lrows = (!lean && n1 - 1 >= PGM_LK_MIN_ROWS && n2 - 1 >= 4 * PGM_LK_T) ? (n1 - 1 + PGM_LK_T - 1) / PGM_LK_T : 0u;
    o.lcols = (n2 - 1 + PGM_LK_T - 1) / PGM_LK_T;
    o.ltab = L.W.take(std::max<size_t>((size_t)o.lrows * PGM_LK_W * PGM_LK_TAB * 2, 16), 256);
    o.lready = L.sync_ints;                              // tiles complete per grid row, then the claim counter and the walker's row (zeroed with the progress counters)
    L.sync_ints += ((size_t)o.lrows + 2 + 3) / 4 * 4;
}
// A plain chain 0 -> 1 -> ... -> n-1 with finite edge costs and no repeat edges (a sequence graph).  Decided before the layout
// pass because jobs of two such graphs get the lean sweep's storage (R rows per lane, code bytes, matrices only on request);
// anything else — also a chain with a missing or infinite edge — takes the general path.
static bool graph_is_chain(const pgm_graph *g) {
    if (g->r_rowptr && g->r_rowptr[g->n] != 0) return false;
    if (g->e_rowptr[0] != 0 || g->e_rowptr[1] != 0) return false;
    for (uint32_t v = 1; v < g->n; ++v) {   // exactly the edge v-1 -> v, at finite cost (stored value 0 means +inf, Graph.h:223-231)
        const int32_t eb = g->e_rowptr[v], ee = g->e_rowptr[v + 1];
        if (eb < 0 || ee - eb != 1 || g->e_col[eb] != v - 1 || g->e_val[eb] == 0.0f) return false;
    }
    return true;
}


// upper bound of the flattened input of one graph side with n nodes and E edges (regular + repeat)
static size_t side_bound_bytes(size_t n, size_t dim, size_t E) {
    E = std::max<size_t>(E, 1);
    return n * dim * 8 + n * sizeof(PgmNode2) + 3 * (n + 1) * 4 + E * 28 + 8 * (size_t)PGM_OV_REC * PGM_OV_ENT + 16 * 16;
}
static size_t model_bound_bytes(size_t dim) { return (dim * dim + dim) * 8 + 64; }

// ---- pass 1: validation, sizes, device layouts -------------------------------------------------
static const pgm_site_ref *site_ref_of(const pgm_site_ref *r, uint32_t i) { return (r && r[i].dev_sites) ? &r[i] : nullptr; }
static bool job_is_two_chains(const pgm_graph *a, const pgm_graph *c) {
    return a && c && a->n >= 2 && c->n >= 2 && a->e_rowptr && c->e_rowptr && a->e_col && c->e_col && a->e_val && c->e_val && graph_is_chain(a) && graph_is_chain(c);
}

// The batch-wide values of the planning, from the jobs' sizes alone (n1, n2, dim, lean).
struct BatchPrologue {
    // The prep and emission kernels are instantiated once per batch for its largest alphabet and read every job's converted
    // profiles with that padded stride: all jobs of a batch get it, whatever their own alphabet (alphabet_tier).
    uint32_t batch_dp = 4u;
    // (the chain of sweeps the batch's largest job would have in pgm_crit_kernel, from the sizes alone: what the other jobs' chains are held against)
    double longest_crit_chain = 0.0;
    // A batch that would not fill the device as MODE 2 sweeps (one band per CU: 0.42 us per step of every band) — a guide-tree level of
    // 16 or 32 jobs on its own, not the 255 jobs of a whole pass — is bound by its longest chain of sweeps, and that chain is 2-3 x
    // shorter in pgm_crit_kernel than on a wavefront of pgm_band_kernel: every job of 8 bands or more goes there then (levels 3 and 4
    // of the headline family alone: 2.05 -> 1.56 and 2.29 -> 1.40 ms per call; level 2, 64 jobs, would fill the device 1.6 times over
    // and stays: 2.2 against 2.4 ms).
    uint32_t promote_bands = 0xffffffffu;
};
static BatchPrologue plan_batch_prologue(const std::vector<PgmJob> &jobs, uint32_t cus) {
    BatchPrologue P;
    uint32_t batch_dim = 0;
    double crit_load = 0.0;
    for (const PgmJob &J : jobs) {
        batch_dim = std::max(batch_dim, J.dim);
        P.longest_crit_chain = std::max(P.longest_crit_chain, ((double)(row_bands(J.n1) - 1) * kLagCritEst + (double)(J.n2 - 1 + 63)) * kTauCrit);
        if (!J.lean) crit_load += (double)row_bands(J.n1) * (double)(J.n2 - 1 + 63) * kTauCrit;
    }
    P.batch_dp = alphabet_tier(batch_dim);
    if (crit_load <= 1.25 * (double)cus * P.longest_crit_chain) P.promote_bands = 8u;
    return P;
}

struct BatchSizes {
    BatchPrologue pro;
    BatchLayout L;
    std::vector<JobOff> off;
    std::vector<size_t> in_base;   // upper bound of the flattened inputs of the jobs before job i (the jobs' slices of the input image)
    uint32_t maxdim = 0, maxnb = 0, maxn = 0, maxnblk = 0;
    uint64_t cells = 0;
};
// pass 1 (serial, O(jobs)): sizes, device layouts, and an upper bound of each job's flattened input.  two_chains[i]: both graphs
// of job i are chains (job_is_two_chains).  Returns the index of the first invalid job, -1 if there is none.
static int plan_sizes(uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2, const pgm_model *const *model, const pgm_scores *scores,
                      uint32_t flags, const pgm_site_ref *res1, const pgm_site_ref *res2, const std::vector<char> &two_chains, uint32_t cus,
                      std::vector<PgmJob> &jobs, BatchSizes &Z) {
    auto side_bound = [](const pgm_graph *g, const pgm_site_ref *res) -> size_t {
        const size_t n = g->n;
        size_t E = (size_t)std::max(0, g->e_rowptr ? g->e_rowptr[n] : 0);
        if (g->r_rowptr) E += (size_t)std::max(0, g->r_rowptr[n]);
        const size_t full = side_bound_bytes(n, g->dim, E);
        return (res && res->dev_sites) ? full - n * g->dim * 8 + n * 4 + 16 : full;   // (resident profiles: a map of n words instead)
    };
    jobs.resize(njobs);
    Z.off.resize(njobs);
    Z.in_base.assign(njobs + 1, 0);
    for (uint32_t i = 0; i < njobs; ++i) {
        const pgm_graph *a = g1[i], *c = g2[i];
        if (!a || !c || !model[i] || a->dim != c->dim || a->dim == 0 || a->dim > PGM_MAX_DIM || a->n < 2 || c->n < 2 || !model[i]->M || !model[i]->pi ||
            (!a->sites && !site_ref_of(res1, i)) || !a->e_rowptr || (!c->sites && !site_ref_of(res2, i)) || !c->e_rowptr)
            return (int)i;
        PgmJob &J = jobs[i];
        memset(&J, 0, sizeof J);
        J.n1 = a->n; J.n2 = c->n; J.dim = a->dim;
        J.ncol = c->n - 1;
        J.tsteps = J.ncol + 63;
        // chain-only jobs: the lean sweep, R = 2 rows per lane (pgm_lean_kernel<2>; the band's buffer descriptor must stay below 1 GiB: see pgm_sweep_chain)
        constexpr uint32_t lean_rshift = 1u;
        J.lean = (two_chains[i] && ((uint64_t)J.tsteps * 1024u << lean_rshift) < (1ull << 30)) ? 1u : 0u;
        J.rshift = J.lean ? lean_rshift : 0u;
        J.nb = (a->n - 1 + (PGM_ROWS << J.rshift) - 1) / (PGM_ROWS << J.rshift);
        J.nblk = (J.tsteps + PGM_BLOCK - 1) / PGM_BLOCK;
        J.maxn = std::max(a->n, c->n);
        J.sc = scores[i];
        J.keep_cells = (!J.lean || (flags & PGM_BATCH_KEEP_MATRICES)) ? 1u : 0u;
        Z.maxnblk = std::max(Z.maxnblk, J.nblk);
        Z.maxn = std::max(Z.maxn, J.maxn);
        Z.maxdim = std::max(Z.maxdim, a->dim);
        Z.maxnb = std::max(Z.maxnb, J.nb << J.rshift);   // (bands of the emission kernel: R virtual bands per band)
        Z.cells += (uint64_t)(a->n - 2) * (c->n - 2);
        Z.in_base[i + 1] = Z.in_base[i] + side_bound(a, site_ref_of(res1, i)) + side_bound(c, site_ref_of(res2, i)) + model_bound_bytes(a->dim);
    }
    Z.pro = plan_batch_prologue(jobs, cus);
    for (uint32_t i = 0; i < njobs; ++i) {
        PgmJob &J = jobs[i];
        J.dp = Z.pro.batch_dp;
        layout_job(Z.L, J.n1, J.n2, J.dp, J.rshift, J.lean != 0, J.keep_cells != 0, Z.off[i]);
    }
    return -1;
}

// ---- pass 2, per job: the sweep a job gets and the LDS of its sweeping wavefront --------------
// Input: the job's sizes (pass 1) and the summaries of its two sides after flatten_side; finishes the flattening (finalize_side, on the
// input image at `base`) and fills the planning fields of the descriptor.  false: graph_is_chain and flatten_side disagree (cannot happen).
static bool plan_job_sweep(PgmJob &J, uint8_t *base, SideOff &s1, SideOff &s2, const BatchPrologue &P) {
    J.has_extras = (s1.nodes_with_extras + s2.nodes_with_extras) > 0 ? 1u : 0u;
    if (J.lean && J.has_extras) return false;
    // LDS of one sweeping wavefront: W / Y history of hD steps x (64 lanes + 16 virtual lanes), X history of hDX
    // steps x 64 lanes, 128 column summaries.  A pair (y - dy, x - dx) is read dy + dx steps back and the virtual
    // lanes are written a block ahead: hD >= maxd1 + maxd2 + 8, hDX >= maxd2 + 1 (powers of two).
    uint32_t hD = 16, hDX = 4;
    while (hD < s1.maxd_kf8 + s2.maxd_kf8 + (uint32_t)PGM_BLOCK) hD *= 2;
    while (hDX < s2.maxd_kf8 + 1) hDX *= 2;
    // history, column ring (5 or 3 float4 per column) and, in a MODE 2 sweep, the helper area behind them
    auto slot_head = [&](bool mode2) { return 2u * hD * (64u + PGM_VL) * 4u + hDX * 64u * 4u + PGM_NRING * (mode2 ? 80u : 48u); };
    // Jobs on the batch's critical path (many bands, or a deep history that leaves room for one or two sweeps per
    // worker anyway) and jobs with edges longer than the on-chip history are swept one band per worker: the other
    // three wavefronts take every term but the chain terms off the sweeping wavefront (pgm_terms_helper), which
    // shortens its step by a factor of 2-3, and serve the long edges from the cell storage with a prefetch.
    const uint32_t nb_job = row_bands(J.n1);
    // (the helpers address the job's cell storage with 32-bit byte offsets)
    const bool allow_long = (uint64_t)J.nb * J.tsteps * 1024u < (1ull << 32);
    const bool has_long = (s1.has_long | s2.has_long) != 0 && allow_long;
    // (a job whose self-contained sweep fits a quarter of the LDS and that is not on the critical path — fewer than 20 bands —
    // goes to pgm_band_kernel's WIDE workers, four bands per CU, instead of one band per CU with helper wavefronts)
    // ... provided its chain of self-contained sweeps (slower per step the more of its nodes have far edges: 0.75 us at none,
    // 1 us at 2.5 %, measured on levels 4 and 5 of the headline family) still ends well before the batch's longest chain
    const double far_density = 0.5 * ((double)s1.cp[J.n1] / J.n1 + (double)s2.cp[J.n2] / J.n2);
    const double chain_wide = ((double)(nb_job - 1) * kLagWideEst + (double)(J.n2 - 1 + 63)) * (0.7 + 10.0 * far_density);
    const bool fits_wide = slot_head(false) <= kWideSlot && chain_wide <= 0.9 * P.longest_crit_chain;
    J.mode2 = (J.has_extras && ((hD >= kMode2MinHd && !fits_wide) || nb_job >= kMode2MinBands || nb_job >= P.promote_bands || has_long)) ? 1u : 0u;
    const bool mode2 = J.mode2 != 0;
    if (mode2) {   // (a MODE 2 sweep keeps every on-chip distance of the graphs, whatever the number of entries of a node)
        while (hD < s1.maxd_cap + s2.maxd_cap + (uint32_t)PGM_BLOCK) hD *= 2;
        while (hDX < s2.maxd_cap + 1) hDX *= 2;
    }
    const uint32_t aux_bytes = mode2 ? (uint32_t)PGM_AUX_BYTES : 0u;
    finalize_side(base, J.n1, s1, 0, mode2, allow_long, false);
    finalize_side(base, J.n2, s2, 1, mode2, allow_long, slot_head(mode2) + aux_bytes + kOvBytes <= (uint32_t)PGM_POOL);
    J.nov2 = mode2 ? s2.nov : 0u;
    J.has_far = (s1.far_nodes + s2.far_nodes) > 0 ? 1u : 0u;
    J.long1 = (mode2 && s1.remote) ? 1u : 0u;
    J.long2 = (mode2 && s2.remote) ? 1u : 0u;
    // MODE 2 jobs whose every predecessor is near or in the LDS history (no long / remote entries, no overflow columns, no
    // generic nodes) are swept by pgm_crit_kernel: the chain terms on one wavefront, everything else on fifteen others
    // (and no interior node without predecessors: the chain wavefront carries no code for them)
    const bool c3 = mode2 && !J.long1 && !J.long2 && J.nov2 == 0 && s1.ngeneric + s2.ngeneric == 0 && s1.nkill + s2.nkill == 0 &&
                    slot_head(true) + aux_bytes + kC3Bytes <= (uint32_t)PGM_POOL;
    if (c3 && hDX < 8u) hDX = 8u;   // (the chain wavefront addresses a block of eight steps from one base: no ring wraps inside a block)
    // the slot, in order: history and column ring, helper area, overflow table, remote rows' rings, the crit3 area
    J.hD = hD; J.hDX = hDX;
    J.slot_bytes = slot_head(mode2);
    J.aux_off = J.slot_bytes;
    J.slot_bytes += aux_bytes;
    J.ov_off = J.slot_bytes;
    if (J.nov2) J.slot_bytes += kOvBytes;
    J.rh_off = J.slot_bytes;
    if (J.long1 | J.long2) J.slot_bytes += 3u * 32u * 64u * 4u;   // W of the last 32 columns of every remote row's walk (one ring per row helper)
    J.c3_off = J.slot_bytes;
    J.crit3 = (c3 && J.slot_bytes + kC3Bytes <= (uint32_t)PGM_POOL) ? 1u : 0u;   // (always fits: hD <= 64, and the deeper X history adds 1 KB)
    if (J.crit3) J.slot_bytes += kC3Bytes;
    J.far_slack = std::max(1u, std::min(4u, std::min(s1.far_dmin, s2.far_dmin)));
    J.nslots = mode2 ? 1u : std::max(1u, std::min((uint32_t)PGM_WAVES, (uint32_t)PGM_POOL / J.slot_bytes));
    if (J.lean) J.nslots = PGM_WAVES;
    return true;
}

// One job of pass 2: both graphs and the model flattened into the job's slice [lo, hi) of the input image at `base`, its sweep planned.
static bool plan_flatten_job(uint8_t *base, size_t lo, size_t hi, const pgm_graph *a, const pgm_graph *c, const pgm_model *m,
                             const pgm_site_ref *r1, const pgm_site_ref *r2, const BatchPrologue &P, PgmJob &J, JobOff &o) {
    Arena A;
    A.base = base; A.off = lo; A.end = hi;
    if (flatten_side(a, J.sc, A, o.s1, r1) != PGM_OK || flatten_side(c, J.sc, A, o.s2, r2) != PGM_OK) return false;
    if (!plan_job_sweep(J, base, o.s1, o.s2, P)) return false;
    o.M = A.put(m->M, sizeof(double) * J.dim * J.dim);
    o.pi = A.put(m->pi, sizeof(double) * J.dim);
    return !A.overflow;
}

// ---- the schedule of a batch ---------------------------------------------------------------------

// How the CUs of the device are dealt to the launches of a batch's fill stage (pure arithmetic; pgm_test_cu_shares exports it for
// the CPU tests).  Every launch is a grid of persistent workers, one per CU, and all of them are resident together (no grid ever
// waits for a CU: pgm_tb_kernel's header says why), so the shares add up to at most `cus` and every queue with work gets at least one.
//   crit   the launch of the longest chains: one CU per band, at most half of the device, and only if it leaves every other
//          queue with work at least one CU (else 0: the caller leaves those jobs in the main launch)
//   then the time to beat is t_goal = max(longest chain of sweeps, all other work / the other CUs).  A batch bound by that chain
//   (chain >= 1.5 x the parallel time) wants the other launches' traffic out of the chain's way early: the lean queue gets the
//   fewest CUs with which it ends within 0.6 t_goal, the band queue within 0.75 t_goal (measured on the headline batch, round 3);
//   a batch bound by throughput wants every queue to end together: the factors go to 1 as the chain's lead shrinks to nothing.
//   rest   the main launch: what is left, never less than its own work needs to end within t_goal — if the shares do not fit,
//          they are cut back in proportion.
struct CuShares { uint32_t lean, band, crit, rest, rest_need; double t_goal, fl, fb; };
static CuShares cu_shares(uint32_t cus, double lean_cost, uint32_t nlean, double band_cost, uint32_t nbands, double rest_cost, uint32_t nrest, uint32_t ncrit, double rsweep) {
    CuShares r = {0u, 0u, 0u, 0u, 0u, 0.0, 1.0, 1.0};
    cus = std::max(1u, cus);
    const uint32_t queues = (nlean != 0) + (nbands != 0) + (nrest != 0);
    if (ncrit != 0 && cus > queues) r.crit = std::min(std::min(ncrit, cus / 2u), cus - queues);
    const uint32_t cap = std::max(1u, cus - r.crit);
    const double sum = (nlean ? lean_cost : 0.0) + (nbands ? band_cost : 0.0) + (nrest ? rest_cost : 0.0);
    const double t_par = std::max(1e-3, sum / cap);
    r.t_goal = std::max(std::max(rsweep, t_par), 1e-3);
    const double w = std::min(1.0, std::max(0.0, (rsweep / t_par - 1.0) / 0.5));
    r.fl = 1.0 - 0.4 * w; r.fb = 1.0 - 0.25 * w;
    auto need = [](double cost, double t, uint32_t most) { return (uint32_t)std::min<double>(most, std::max(1.0, std::ceil(cost / t))); };
    const uint32_t band_most = (nbands + PGM_WAVES - 1) / PGM_WAVES;
    uint32_t lean = nlean ? need(lean_cost, r.fl * r.t_goal, nlean) : 0u, band = nbands ? need(band_cost, r.fb * r.t_goal, band_most) : 0u;
    uint32_t rest = nrest ? need(rest_cost, r.t_goal, nrest) : 0u;
    if (lean + band + rest > cap) {   // cut back in proportion to the work, at least one CU each (cap >= queues unless the device has fewer CUs than queues)
        const double scale = (double)cap / (double)(lean + band + rest);
        auto cut = [&](uint32_t v) { return v ? std::max(1u, (uint32_t)std::floor(v * scale)) : 0u; };
        lean = cut(lean); band = cut(band); rest = cut(rest);
        while (lean + band + rest > cap) {   // (rounding up to one CU each)
            uint32_t *big = &rest; if (band > *big) big = &band; if (lean > *big) big = &lean;
            if (*big <= 1u) break;
            --*big;
        }
    }
    r.rest_need = rest;
    const uint32_t left = cap > lean + band + rest ? cap - lean - band - rest : 0u;
    if (nrest) rest = std::min(nrest, rest + left);          // the main launch takes what is left ...
    else if (nbands) band = std::min(band_most, band + left);   // ... or the band queue, or the lean queue
    else if (nlean) lean = std::min(nlean, lean + left);
    r.lean = lean; r.band = band; r.rest = rest;
    return r;
}

// The work lists of a batch's fill stage, their order, and the workers (CUs) of every launch.
struct BatchSchedule {
    std::vector<PgmItem> items;       // the fill work list: the first ncrit items are the launch of the longest chains, the rest the main launch
    std::vector<PgmItem> bands;       // pgm_band_kernel's list, one band per entry: the first nbands_narrow fit an eighth of a CU's LDS, the rest a quarter
    std::vector<uint32_t> lean_list;  // pgm_lean_kernel's queue, largest job first
    std::vector<int2> tblist;         // the jobs of the main launch (largest first), of the launch of the longest chains, of the band kernel: (job, its last item of the work list)
    uint32_t nitems = 0, nbands = 0, nlean = 0;   // entries of the lists (an empty bands, lean_list or tblist holds one unused entry: their uploads are never empty)
    uint32_t ncrit = 0, nbands_narrow = 0, ntb = 0, ntb_c = 0, ntb_b = 0;
    uint32_t nworkers = 0, nlean_workers = 0, nband_workers = 0, nwide_workers = 0, ncrit_workers = 0, ntb_workers = 0, ntb_b_workers = 0;
    bool crit_c3 = false, rest_c3 = false;   // every item of the launch for the longest chains / of the main launch belongs to a crit3 job: pgm_crit_kernel sweeps that list
    // what the PGM_HOST_PROFILE "work lists:" line prints
    double rsweep = 0, t_goal = 0, lean_cost = 0, band_cost = 0, band_end = 0, other_cost = 0, fill_end = 0, crit_end = 0;
    size_t total_b = 0, total = 0, total_c = 0;
    uint32_t capacity = 0;            // the main launch's CUs
};

struct SimItem { double rem, dur, gap; uint32_t job, band, count; };
// Event simulation of `workers` persistent workers over the items of the jobs pj (ascending within a job), `count` in all: free
// workers (min-heap of times), ready items (max-heap of remaining paths), pending successors.  Writes the order in which the
// workers take the items (with their wave priorities, against the batch's longest remaining path rmax) and returns the end.
static double simulate_workers(const std::vector<std::vector<SimItem>> &pj, size_t count, uint32_t workers, double rmax, std::vector<PgmItem> &out) {
    out.clear();
    double end = 0.0;
    typedef std::pair<double, uint32_t> TE;   // (time, job)
    std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
    for (uint32_t w = 0; w < std::max(1u, workers); ++w) free_at.push(0.0);
    std::priority_queue<TE> ready;                                               // (rem, job): next item of that job
    std::priority_queue<TE, std::vector<TE>, std::greater<TE>> pending;         // (ready time, job)
    std::vector<uint32_t> next(pj.size(), 0);
    for (uint32_t i = 0; i < pj.size(); ++i) if (!pj[i].empty()) ready.push({pj[i][0].rem, i});
    out.reserve(count);
    double now = 0.0;
    while (out.size() < count) {
        now = std::max(now, free_at.top());
        while (!pending.empty() && pending.top().first <= now) {
            const uint32_t j = pending.top().second; pending.pop();
            ready.push({pj[j][next[j]].rem, j});
        }
        if (ready.empty()) { now = pending.top().first; continue; }              // every free worker would have to wait
        const uint32_t j = ready.top().second; ready.pop();
        const SimItem &it = pj[j][next[j]];
        // wave priority (s_setprio): the longest paths of the batch win the issue arbitration on their SIMDs
        out.push_back(PgmItem{it.job, it.band, it.rem > 0.6 * rmax ? 3u : (it.rem > 0.35 * rmax ? 2u : (it.rem > 0.2 * rmax ? 1u : 0u)), it.count});
        free_at.pop();
        free_at.push(now + it.dur);
        end = std::max(end, now + it.dur);
        // the longest paths of the batch are not held back: their next band gets a worker at once (it spins until the
        // predecessor is far enough, but then follows it without any queueing delay)
        if (++next[j] < pj[j].size()) pending.push({pj[j][next[j]].rem > kEager * rmax ? now : now + it.gap, j});
    }
    return end;
}

// how many of the band queue's `cus` workers sweep the wide bands: by their share of the work, at least one worker for either kind
static uint32_t wide_share(uint32_t cus, size_t total_b, size_t total_w, double wide_cost, double band_cost) {
    if (total_w == 0) return 0u;
    if (total_b == 0) return cus;
    const uint32_t w = (uint32_t)std::lround(cus * wide_cost / band_cost);
    return std::max(1u, std::min(cus > 1u ? cus - 1u : 1u, w));
}

// ---- fill work list.  An item is a band (MODE 2 jobs) or a group of up to eight bands (all others); item k of a job
// can start once item k-1 has been running for the band-to-band lag, and the workers take items in list order.  The
// order is the result of simulating the persistent workers on the host with estimated times: whenever a worker is
// free it takes, among the items that are READY by then, the one with the longest remaining path (the time until its
// job is complete: the lags still ahead, one full sweep, the traceback).  Within a job the items keep ascending
// order, as the kernel requires; taking only ready items keeps workers from idling in front of a predecessor band.
// jobs: the planned descriptors (plan_job_sweep); order: largest job first; cus: persistent workers, one workgroup of 8
// wavefronts per CU (it owns the CU's LDS for its sweeps' histories).
static BatchSchedule plan_schedule(const std::vector<PgmJob> &jobs, const std::vector<uint32_t> &order, uint32_t cus) {
    BatchSchedule S;
    const uint32_t njobs = (uint32_t)jobs.size();
    S.capacity = cus;
    if (njobs) {
        std::vector<std::vector<SimItem>> per_job(njobs), per_job_b(njobs), per_job_c(njobs), per_job_w(njobs);   // main launch, narrow bands, longest chains, wide bands
        std::vector<double> chain_of(njobs, 0.0);   // chain of sweeps of the jobs of the fill kernel
        // The jobs without helper wavefronts go to pgm_band_kernel, band by band (not a job whose sweep would not fit a quarter of the LDS)
        size_t total = 0, total_b = 0, total_w = 0;
        double rmax = 1.0, rsweep = 1.0;   // longest remaining path with / without the traceback behind it
        for (uint32_t q = 0; q < njobs; ++q) {
            const uint32_t i = order[q];   // (largest first: the order of the lean queue)
            const PgmJob &J = jobs[i];
            const double tau = J.crit3 ? kTauCrit : (J.mode2 ? kTauMode2 : (J.has_extras ? kTauExtras : kTauChain));     // us per step
            const double tb = (J.has_extras ? 0.3 : 0.2) * (double)(J.n1 + J.n2);   // the traceback follows the last band (us)
            if (J.lean) {   // pgm_lean_kernel's queue: a worker's wavefronts cycle over the job's bands (72 steps behind each other), then the walk
                const double rounds = std::ceil((double)J.nb / PGM_WAVES), first = std::min<double>(J.nb, PGM_WAVES);
                S.lean_cost += kTauLean * (rounds * J.tsteps + (first - 1.0) * 72.0) + 0.04 * (double)(J.n1 + J.n2);
                S.lean_list.push_back(i);
                continue;
            }
            const bool narrow = !J.mode2 && J.slot_bytes <= kNarrowSlot;
            const bool wide = !J.mode2 && !narrow && J.slot_bytes <= kWideSlot;
            const bool per_band = narrow || wide;
            if (!per_band) chain_of[i] = tau * ((double)(J.nb - 1) * kLag + J.tsteps);
            const uint32_t group = per_band ? 1u : J.nslots;       // bands per item, one per wavefront of the worker
            for (uint32_t band = 0; band < J.nb; band += group) {
                const uint32_t cnt = std::min(group, J.nb - band);
                SimItem it;
                it.rem = tau * ((double)(J.nb - 1 - band) * kLag + J.tsteps) + tb;
                it.dur = tau * ((double)(cnt - 1) * kLag + J.tsteps);   // (the traceback is another kernel's: pgm_tb_kernel)
                it.gap = tau * (double)cnt * kLag;                 // the next item may start this long after this one
                it.job = i; it.band = band; it.count = cnt;
                (wide ? per_job_w : (narrow ? per_job_b : per_job))[i].push_back(it);
                rmax = std::max(rmax, it.rem);
                rsweep = std::max(rsweep, it.rem - tb);
            }
            total += per_job[i].size();
            total_b += per_job_b[i].size();
            total_w += per_job_w[i].size();
        }
        // The CUs are split between the kernels (one worker per CU in each), see cu_shares(): the jobs with the longest chains of
        // sweeps (within 15 % of the longest: the root of a guide tree, as a rule) get a launch of the fill kernel of their own, one CU
        // per band — their tracebacks are the last thing a batch waits for, and this way the other jobs' tracebacks are out of the
        // way before they start (each launch is followed by its own instance of pgm_tb_kernel); only if other jobs stay behind for
        // the main launch.  The rest of the CUs is dealt to the lean queue, the band queue and the main launch by their costs.
        double band_cost = 0.0, crit_cost = 0.0, wide_cost = 0.0, other_cost = 0.0;   // worker-microseconds of the queues
        for (uint32_t i = 0; i < njobs; ++i) {
            for (const SimItem &it : per_job[i]) other_cost += it.dur;
            for (const SimItem &it : per_job_b[i]) band_cost += it.dur / PGM_WAVES;
            for (const SimItem &it : per_job_w[i]) wide_cost += it.dur / PGM_WIDE_WAVES;
        }
        band_cost += wide_cost;   // one queue for the shares: pgm_band_kernel's workers, split below
        auto in_crit = [&](uint32_t i) { return !per_job[i].empty() && chain_of[i] >= 0.85 * rsweep; };
        size_t total_c = 0;
        if (total != 0) {
            uint32_t ncj = 0, nrestj = 0;
            for (uint32_t i = 0; i < njobs; ++i) if (!per_job[i].empty()) { if (in_crit(i)) ++ncj; else ++nrestj; }
            if (ncj != 0 && nrestj != 0)
                for (uint32_t i = 0; i < njobs; ++i)
                    if (in_crit(i)) { total_c += per_job[i].size(); for (const SimItem &it : per_job[i]) crit_cost += it.dur; }
        }
        const uint32_t nlean = (uint32_t)S.lean_list.size(), band_units = (uint32_t)(total_b + 2 * total_w);
        CuShares sh = cu_shares(cus, S.lean_cost, nlean, band_cost, band_units, other_cost - crit_cost, (uint32_t)(total - total_c), (uint32_t)total_c, rsweep);
        if (total_c != 0 && sh.crit == 0) {   // no CU to spare for a launch of their own: the longest chains stay in the main launch
            total_c = 0; crit_cost = 0.0;
            sh = cu_shares(cus, S.lean_cost, nlean, band_cost, band_units, other_cost, (uint32_t)total, 0u, rsweep);
        }
        if (total_c != 0)
            for (uint32_t i = 0; i < njobs; ++i)
                if (in_crit(i)) per_job_c[i].swap(per_job[i]);
        total -= total_c;
        const double t_goal = sh.t_goal;
        uint32_t lean_cus = sh.lean, band_cus = sh.band, crit_cus = sh.crit;
        // (a lean job is one worker's: the queue ends after ceil(jobs / workers) rounds — the fewest workers with that many rounds do)
        if (lean_cus) { const uint32_t rounds = (nlean + lean_cus - 1u) / lean_cus; lean_cus = (nlean + rounds - 1u) / rounds; }
        S.nlean_workers = lean_cus;
        double band_end = 0.0;
        uint32_t wide_cus = 0;
        if (total_b + total_w != 0) {
            // (a simulation of a 1000-band list is 0.1 ms: the share grows by how far the simulated schedule overshoots, three times at
            // most, and only into CUs the main launch does not need for its own share).  The share is split between the workers of
            // the narrow bands (eight at a time per CU) and of the wide ones (four at a time) by their work.
            std::vector<PgmItem> bands_w;
            const uint32_t most = std::max(band_cus, band_cus + (sh.rest > sh.rest_need ? sh.rest - sh.rest_need : 0u));
            auto run = [&](uint32_t n) {
                wide_cus = wide_share(n, total_b, total_w, wide_cost, band_cost);
                const uint32_t ncus = n > wide_cus ? n - wide_cus : (total_b ? 1u : 0u);
                double e = 0.0;
                if (total_b) e = simulate_workers(per_job_b, total_b, ncus * PGM_WAVES, rmax, S.bands);
                if (total_w) e = std::max(e, simulate_workers(per_job_w, total_w, wide_cus * PGM_WIDE_WAVES, rmax, bands_w));
                return e;
            };
            if (total != 0) {
                for (int it = 0; it < 3 && band_cus < most; ++it) {
                    band_end = run(band_cus);
                    if (band_end <= sh.fb * t_goal) break;
                    band_cus = std::min(most, std::max(band_cus + 1u, (uint32_t)std::ceil(band_cus * std::min(2.0, band_end / (sh.fb * t_goal)))));
                }
            }
            band_cus = std::max(1u, std::min<uint32_t>(std::min(band_cus, most), (uint32_t)((total_b + PGM_WAVES - 1) / PGM_WAVES + (total_w + PGM_WIDE_WAVES - 1) / PGM_WIDE_WAVES)));
            if (total_b && total_w) band_cus = std::max(band_cus, 2u);
            band_end = run(band_cus);
            if (total_b == 0) S.bands.clear();
            S.nbands_narrow = (uint32_t)S.bands.size();
            S.bands.insert(S.bands.end(), bands_w.begin(), bands_w.end());
            // the tracebacks of the band kernel's jobs follow it on its CUs, one worker per job: with fewer workers than jobs the last ones
            // wait a whole walk longer — a round less if the main launch can spare the CUs for it
            uint32_t nbj = 0;
            for (uint32_t i = 0; i < njobs; ++i) nbj += (!per_job_b[i].empty() || !per_job_w[i].empty());
            const uint32_t most_tb = std::max(band_cus, band_cus + (sh.rest > sh.rest_need ? sh.rest - sh.rest_need : 0u));
            if (nbj > band_cus) {
                const uint32_t rounds = (nbj + band_cus - 1u) / band_cus, want = rounds > 1u ? (nbj + rounds - 2u) / (rounds - 1u) : band_cus;
                if (want > band_cus && want <= most_tb && want <= band_cus + band_cus / 8u + 1u) {
                    band_cus = want;
                    wide_cus = wide_share(band_cus, total_b, total_w, wide_cost, band_cost);
                }
            }
        }
        S.nwide_workers = wide_cus;
        S.nband_workers = band_cus;
        if (total_c != 0) {
            // the launch of the longest chains has a worker per band — but a job never has more than tsteps / lag + 2 of its bands under way
            // at the same time (the first are through before the last may start): the workers beyond that go to the main launch
            uint32_t need = 0;
            for (uint32_t i = 0; i < njobs; ++i)
                if (!per_job_c[i].empty()) need += std::min<uint32_t>(jobs[i].nb, jobs[i].tsteps / (uint32_t)std::max(1.0, kLag) + 2u);
            crit_cus = std::max(1u, std::min(crit_cus, need));
        }
        S.capacity = std::max(1u, cus > lean_cus + band_cus + crit_cus ? cus - lean_cus - band_cus - crit_cus : 1u);
        S.ncrit_workers = crit_cus;
        std::vector<PgmItem> items_rest;
        S.crit_end = total_c ? simulate_workers(per_job_c, total_c, crit_cus, rmax, S.items) : 0.0;
        S.ncrit = (uint32_t)S.items.size();
        S.fill_end = simulate_workers(per_job, total, S.capacity, rmax, items_rest);
        S.items.insert(S.items.end(), items_rest.begin(), items_rest.end());
        S.rsweep = rsweep; S.t_goal = t_goal; S.band_cost = band_cost; S.band_end = band_end; S.other_cost = other_cost;
        S.total_b = total_b; S.total = total; S.total_c = total_c;
    }
    S.nitems = (uint32_t)S.items.size(); S.nbands = (uint32_t)S.bands.size(); S.nlean = (uint32_t)S.lean_list.size();
    S.nworkers = std::max(1u, std::min(S.capacity, S.nitems - S.ncrit));
    S.crit_c3 = S.ncrit != 0; S.rest_c3 = S.nitems > S.ncrit;
    std::vector<int> last_item(njobs, 0), group(njobs, 0);
    for (uint32_t k = 0; k < S.nitems; ++k) {
        const PgmItem &it = S.items[k];
        if (!jobs[it.job].crit3) (k < S.ncrit ? S.crit_c3 : S.rest_c3) = false;
        if (it.band + it.count == jobs[it.job].nb) last_item[it.job] = (int)k;
        if (k < S.ncrit) group[it.job] = 1;
    }
    for (const PgmItem &it : S.bands) group[it.job] = 2;
    uint32_t cnt[3] = {0, 0, 0};
    for (int pass = 0; pass < 3; ++pass)
        for (uint32_t q = 0; q < njobs; ++q) { const uint32_t i = order[q]; if (!jobs[i].lean && group[i] == pass) { S.tblist.push_back(make_int2((int)i, last_item[i])); ++cnt[pass]; } }
    S.ntb = cnt[0]; S.ntb_c = cnt[1]; S.ntb_b = cnt[2];
    // workers of the traceback instances: the CUs of the kernel each instance follows (they are free by then; nothing of either
    // grid is left waiting for a CU while other kernels of the batch still run)
    const uint32_t all_cus = std::max(1u, cus) - S.nlean_workers;
    S.ntb_workers = std::max(1u, (S.ntb_b || S.ntb_c) ? S.nworkers : all_cus);
    S.ntb_b_workers = std::max(1u, (S.ntb || S.ntb_c) ? S.nband_workers : all_cus);
    if (S.bands.empty()) S.bands.push_back(PgmItem{0u, 0u, 0u, 0u});
    if (S.lean_list.empty()) S.lean_list.push_back(0u);
    if (S.tblist.empty()) S.tblist.push_back(make_int2(0, 0));
    return S;
}

}  // namespace

#endif
