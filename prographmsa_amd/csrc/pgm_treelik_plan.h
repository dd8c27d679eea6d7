// pgm_treelik_plan.h — where everything of a tree-likelihood call lies in the five scratch slots the eight entries share
// (pgm_tree_likelihood, pgm_tree_likelihood_rates, pgm_tree_ancestral, pgm_tree_nni, pgm_tree_nni_edge, pgm_tree_spr,
// pgm_tree_ancestral_joint, pgm_tree_ancestral_sample; pgm_treelik_capi.inc fills the kernels' arguments from it).  Plain C++17 without HIP types: the host compiler takes it alone (tests/test_cpu_treelik_plan.py).
//
// A region is absent (0 bytes) where the call has no use for it.  The regions of a slot follow each other in the order of the list
// below, each at the next multiple of its alignment; a slot ends where its last region ends.  C = ncat (1 in the plain entry),
// X = 3 with derivs, else 1.  "nni" is both pgm_tree_nni and pgm_tree_nni_edge; "edge" the latter alone, whose per-site ratios,
// chunk sums and sums are those of its candidates, so they take the regions of the edges' (G, H, PART, D1, D2: never both in a call).
// "spr" is pgm_tree_spr: the walk's regions of nni (U, O, CL, CK, the outputs, RHO) and three of its own behind the others of their slot.
// "joint" is pgm_tree_ancestral_joint, "sample" pgm_tree_ancestral_sample: the regions of rates without derivs and their own behind them.
//   TREE  CHILD   uint32  (nnodes + 1) + nedges      child_off, then child: the children of every node, ascending
//         PI      double  dim
//         W       double  ncat                       all but plain
//         PARENT  uint32  nnodes                     nni, joint, sample
//         CAND    uint32  3 x ncand                  nni: cand_v, cand_a, cand_c
//         ROWS    int8    nleaves x ncols
//         SPR_CAND uint32 ncand                      spr: cand_v (y is the last node of the candidate's path)
//         SPR_PATH uint32 PGM_TREELIK_SPR_STRIDE x ncand   spr: per candidate J, M and the nodes of its path (pgm_treelik_check.h)
//   P     P       double  C x nedges x X x dim x dim
//         PC      double  ncat x ncand x 3 x dim x dim   edge: the candidates' own matrices
//         PH      double  ncat x nedges x dim x dim  spr: the matrix of half of every edge
//   U     U       double  C x ninner x ncols x dim   the partials
//         O       double  as U                       derivs, ancestral (the posteriors take their place), nni: the outside vectors
//         JF      double  ninner x ncols x dim       joint: F of the max pass, under the site's category
//         JPTR    uint8   ninner x dim x ncols       joint: the back-pointers, the sites fastest
//   G     CL      double  ncat x ncols               all but plain: L_c of every category
//         CK      int32   ncat x ncols               all but plain: k_c
//         GC, QC  double  ncat x nedges x ncols      rates with derivs: g_c, q_c
//         G, H    double  nedges x ncols             derivs: the per-site ratios (rates: the mixed ones); edge: ncand x ncols
//         PART    double  2 x nedges x nchunks       derivs: the chunk sums; edge: 2 x ncand x nchunks
//   OUT   SITE_L  double  ncols
//         SITE_K  int32   ncols
//         POST    double  ncat x ncols               all but plain
//         D1, D2  double  nedges                     derivs; edge: ncand
//         ANC_PROB double ninner x ncols             ancestral
//         ANC_STATE int8  ninner x ncols             ancestral
//         ANC_POST double ninner x ncols x dim       ancestral, when asked for
//         RHO     double  ncand x ncols              nni, spr
//         JL      double  ncols                      joint: joint_l
//         JK      int32   ncols                      joint: joint_k
//         JCAT    uint8   ncols                      joint: cat
//         JSTATE  int8    ninner x ncols             joint: joint_state
//         SCAT    uint8   ncols x nsamp              sample: samp_cat
//         SSTATE  int8    ninner x ncols x nsamp     sample: samp_state
#ifndef PGM_TREELIK_PLAN_H_
#define PGM_TREELIK_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "../../include/pgm_hip.h"
#include "pgm_treelik_check.h"

enum { PGM_TREELIK_CALL_PLAIN = 0, PGM_TREELIK_CALL_RATES, PGM_TREELIK_CALL_ANC, PGM_TREELIK_CALL_NNI, PGM_TREELIK_CALL_NNI_EDGE, PGM_TREELIK_CALL_SPR,
       PGM_TREELIK_CALL_JOINT, PGM_TREELIK_CALL_SAMPLE };
enum { PGM_TL_SLOT_TREE = 0, PGM_TL_SLOT_P, PGM_TL_SLOT_U, PGM_TL_SLOT_G, PGM_TL_SLOT_OUT, PGM_TL_NSLOTS };   // the order of pgm_ctx's SC_TREELIK_*
enum {
    PGM_TL_CHILD = 0, PGM_TL_PI, PGM_TL_W, PGM_TL_PARENT, PGM_TL_CAND, PGM_TL_ROWS,
    PGM_TL_P,
    PGM_TL_U, PGM_TL_O,
    PGM_TL_CL, PGM_TL_CK, PGM_TL_GC, PGM_TL_QC, PGM_TL_G, PGM_TL_H, PGM_TL_PART,
    PGM_TL_SITE_L, PGM_TL_SITE_K, PGM_TL_POST, PGM_TL_D1, PGM_TL_D2, PGM_TL_ANC_PROB, PGM_TL_ANC_STATE, PGM_TL_ANC_POST, PGM_TL_RHO,
    PGM_TL_NREGIONS,                      // the regions the four first modes have between them
    PGM_TL_PC = PGM_TL_NREGIONS,          // pgm_tree_nni_edge's own, numbered behind them
    PGM_TL_PH, PGM_TL_SPR_CAND, PGM_TL_SPR_PATH,   // pgm_tree_spr's own
    PGM_TL_JF, PGM_TL_JPTR, PGM_TL_JL, PGM_TL_JK, PGM_TL_JCAT, PGM_TL_JSTATE,   // pgm_tree_ancestral_joint's own
    PGM_TL_SCAT, PGM_TL_SSTATE,                    // pgm_tree_ancestral_sample's own
    PGM_TL_NREGIONS_ALL
};

struct PgmTreelikRegion { uint32_t slot, align; size_t off, bytes; };   // (bytes == 0: absent)
struct PgmTreelikPlan {
    uint32_t nedges, ninner, cats;                                  // cats: ncat, 1 in the plain entry
    size_t mat, nrow, nchunks, npairs;                              // dim x dim; nleaves x ncols; chunks of sites; ninner x ncols
    size_t p_count, u_count, g_count, cl_count;                     // doubles of one category's matrices, partials, ratios; ncat x ncols
    size_t slot_bytes[PGM_TL_NSLOTS];
    PgmTreelikRegion r[PGM_TL_NREGIONS_ALL];
};

// ncat: 0 for the plain entry; derivs: plain and rates alone; ncand: nni, nni edge and spr alone; full: ancestral alone, anc_post asked for;
// nsamp: sample alone
inline PgmTreelikPlan pgm_treelik_plan(int mode, uint32_t dim, uint32_t nleaves, uint32_t nnodes, uint32_t ncols, uint32_t ncat, bool derivs, uint32_t ncand, bool full,
                                       uint32_t nsamp = 0) {
    PgmTreelikPlan p = {};
    const bool joint = mode == PGM_TREELIK_CALL_JOINT, sample = mode == PGM_TREELIK_CALL_SAMPLE;
    const bool edge = mode == PGM_TREELIK_CALL_NNI_EDGE, nni = mode == PGM_TREELIK_CALL_NNI || edge;
    const bool spr = mode == PGM_TREELIK_CALL_SPR;
    const bool cats = mode != PGM_TREELIK_CALL_PLAIN, outside = derivs || mode == PGM_TREELIK_CALL_ANC || nni || spr;
    p.nedges = nnodes - 1; p.ninner = nnodes - nleaves; p.cats = cats ? ncat : 1;
    p.mat = (size_t)dim * dim; p.nrow = (size_t)nleaves * ncols; p.nchunks = ((size_t)ncols + PGM_TREELIK_CHUNK - 1) / PGM_TREELIK_CHUNK;
    p.npairs = (size_t)p.ninner * ncols;
    p.p_count = p.mat * (derivs ? 3 : 1) * p.nedges; p.u_count = p.npairs * dim; p.g_count = derivs ? (size_t)p.nedges * ncols : 0;
    p.cl_count = cats ? (size_t)ncat * ncols : 0;
    auto put = [&p](int region, uint32_t slot, uint32_t align, size_t bytes) {
        if (bytes == 0) return;
        const size_t off = (p.slot_bytes[slot] + align - 1) / align * align;
        p.r[region] = {slot, align, off, bytes};
        p.slot_bytes[slot] = off + bytes;
    };
    put(PGM_TL_CHILD, PGM_TL_SLOT_TREE, 4, 4 * ((size_t)nnodes + 1 + p.nedges));
    put(PGM_TL_PI, PGM_TL_SLOT_TREE, 8, 8 * (size_t)dim);
    put(PGM_TL_W, PGM_TL_SLOT_TREE, 8, cats ? 8 * (size_t)ncat : 0);
    put(PGM_TL_PARENT, PGM_TL_SLOT_TREE, 4, nni || joint || sample ? 4 * (size_t)nnodes : 0);
    put(PGM_TL_CAND, PGM_TL_SLOT_TREE, 4, nni ? 12 * (size_t)ncand : 0);
    put(PGM_TL_ROWS, PGM_TL_SLOT_TREE, 1, p.nrow);
    put(PGM_TL_SPR_CAND, PGM_TL_SLOT_TREE, 4, spr ? 4 * (size_t)ncand : 0);
    put(PGM_TL_SPR_PATH, PGM_TL_SLOT_TREE, 4, spr ? 4 * (size_t)PGM_TREELIK_SPR_STRIDE * ncand : 0);
    put(PGM_TL_P, PGM_TL_SLOT_P, 8, 8 * p.p_count * p.cats);
    put(PGM_TL_PC, PGM_TL_SLOT_P, 8, edge ? 8 * 3 * p.mat * ncand * ncat : 0);
    put(PGM_TL_PH, PGM_TL_SLOT_P, 8, spr ? 8 * p.p_count * p.cats : 0);
    put(PGM_TL_U, PGM_TL_SLOT_U, 8, 8 * p.u_count * p.cats);
    put(PGM_TL_O, PGM_TL_SLOT_U, 8, outside ? 8 * p.u_count * p.cats : 0);
    put(PGM_TL_JF, PGM_TL_SLOT_U, 8, joint ? 8 * p.u_count : 0);
    put(PGM_TL_JPTR, PGM_TL_SLOT_U, 1, joint ? p.u_count : 0);
    put(PGM_TL_CL, PGM_TL_SLOT_G, 8, 8 * p.cl_count);
    put(PGM_TL_CK, PGM_TL_SLOT_G, 4, 4 * p.cl_count);
    put(PGM_TL_GC, PGM_TL_SLOT_G, 8, cats ? 8 * p.g_count * ncat : 0);
    put(PGM_TL_QC, PGM_TL_SLOT_G, 8, cats ? 8 * p.g_count * ncat : 0);
    put(PGM_TL_G, PGM_TL_SLOT_G, 8, edge ? 8 * (size_t)ncand * ncols : 8 * p.g_count);
    put(PGM_TL_H, PGM_TL_SLOT_G, 8, edge ? 8 * (size_t)ncand * ncols : 8 * p.g_count);
    put(PGM_TL_PART, PGM_TL_SLOT_G, 8, edge ? 8 * 2 * (size_t)ncand * p.nchunks : derivs ? 8 * 2 * (size_t)p.nedges * p.nchunks : 0);
    put(PGM_TL_SITE_L, PGM_TL_SLOT_OUT, 8, 8 * (size_t)ncols);
    put(PGM_TL_SITE_K, PGM_TL_SLOT_OUT, 4, 4 * (size_t)ncols);
    put(PGM_TL_POST, PGM_TL_SLOT_OUT, 8, 8 * p.cl_count);
    put(PGM_TL_D1, PGM_TL_SLOT_OUT, 8, edge ? 8 * (size_t)ncand : derivs ? 8 * (size_t)p.nedges : 0);
    put(PGM_TL_D2, PGM_TL_SLOT_OUT, 8, edge ? 8 * (size_t)ncand : derivs ? 8 * (size_t)p.nedges : 0);
    put(PGM_TL_ANC_PROB, PGM_TL_SLOT_OUT, 8, mode == PGM_TREELIK_CALL_ANC ? 8 * p.npairs : 0);
    put(PGM_TL_ANC_STATE, PGM_TL_SLOT_OUT, 1, mode == PGM_TREELIK_CALL_ANC ? p.npairs : 0);
    put(PGM_TL_ANC_POST, PGM_TL_SLOT_OUT, 8, mode == PGM_TREELIK_CALL_ANC && full ? 8 * p.u_count : 0);
    put(PGM_TL_RHO, PGM_TL_SLOT_OUT, 8, nni || spr ? 8 * (size_t)ncand * ncols : 0);
    put(PGM_TL_JL, PGM_TL_SLOT_OUT, 8, joint ? 8 * (size_t)ncols : 0);
    put(PGM_TL_JK, PGM_TL_SLOT_OUT, 4, joint ? 4 * (size_t)ncols : 0);
    put(PGM_TL_JCAT, PGM_TL_SLOT_OUT, 1, joint ? (size_t)ncols : 0);
    put(PGM_TL_JSTATE, PGM_TL_SLOT_OUT, 1, joint ? p.npairs : 0);
    put(PGM_TL_SCAT, PGM_TL_SLOT_OUT, 1, sample ? (size_t)ncols * nsamp : 0);
    put(PGM_TL_SSTATE, PGM_TL_SLOT_OUT, 1, sample ? p.npairs * nsamp : 0);
    return p;
}

#endif
