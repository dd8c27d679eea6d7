// treelik_plan_test.cpp — pgm_treelik_plan (csrc/pgm_treelik_plan.h) with the host compiler alone: for every mode and the shapes at
// which the padding terms matter, every region has the size its contents need, lies inside its slot, overlaps no other and is aligned
// for what it holds, and every slot ends with its last region.  Prints the number of plans checked; exit status 1 and a line per
// finding otherwise.
#include "pgm_treelik_plan.h"

#include <cstdio>
#include <initializer_list>

struct Kind { int region, slot; unsigned align; const char *name; };   // stated here on its own: what a region holds and where
static const Kind kKinds[PGM_TL_NREGIONS] = {
    {PGM_TL_CHILD, PGM_TL_SLOT_TREE, 4, "child"}, {PGM_TL_PI, PGM_TL_SLOT_TREE, 8, "pi"}, {PGM_TL_W, PGM_TL_SLOT_TREE, 8, "w"},
    {PGM_TL_PARENT, PGM_TL_SLOT_TREE, 4, "parent"}, {PGM_TL_CAND, PGM_TL_SLOT_TREE, 4, "cand"}, {PGM_TL_ROWS, PGM_TL_SLOT_TREE, 1, "rows"},
    {PGM_TL_P, PGM_TL_SLOT_P, 8, "P"},
    {PGM_TL_U, PGM_TL_SLOT_U, 8, "U"}, {PGM_TL_O, PGM_TL_SLOT_U, 8, "O"},
    {PGM_TL_CL, PGM_TL_SLOT_G, 8, "L_c"}, {PGM_TL_CK, PGM_TL_SLOT_G, 4, "k_c"}, {PGM_TL_GC, PGM_TL_SLOT_G, 8, "g_c"}, {PGM_TL_QC, PGM_TL_SLOT_G, 8, "q_c"},
    {PGM_TL_G, PGM_TL_SLOT_G, 8, "g"}, {PGM_TL_H, PGM_TL_SLOT_G, 8, "h"}, {PGM_TL_PART, PGM_TL_SLOT_G, 8, "chunk sums"},
    {PGM_TL_SITE_L, PGM_TL_SLOT_OUT, 8, "site_l"}, {PGM_TL_SITE_K, PGM_TL_SLOT_OUT, 4, "site_k"}, {PGM_TL_POST, PGM_TL_SLOT_OUT, 8, "post"},
    {PGM_TL_D1, PGM_TL_SLOT_OUT, 8, "d1"}, {PGM_TL_D2, PGM_TL_SLOT_OUT, 8, "d2"}, {PGM_TL_ANC_PROB, PGM_TL_SLOT_OUT, 8, "anc_prob"},
    {PGM_TL_ANC_STATE, PGM_TL_SLOT_OUT, 1, "anc_state"}, {PGM_TL_ANC_POST, PGM_TL_SLOT_OUT, 8, "anc_post"}, {PGM_TL_RHO, PGM_TL_SLOT_OUT, 8, "rho"},
};

static const char *kSlots[PGM_TL_NSLOTS] = {"TREE", "P", "U", "G", "OUT"};

int main() {
    long plans = 0, findings = 0;
    for (int mode : {PGM_TREELIK_CALL_PLAIN, PGM_TREELIK_CALL_RATES, PGM_TREELIK_CALL_ANC, PGM_TREELIK_CALL_NNI})
    for (uint32_t dim : {1u, 3u, 64u})
    for (uint32_t nleaves : {3u, 4u, 8u})
    for (uint32_t nnodes = nleaves + 1; nnodes <= 2 * nleaves - 1; ++nnodes)   // a star .. a binary tree: odd and even, ninner 1 .. nleaves - 1
    for (uint32_t ncols : {1u, 2u, 15u, 17u})
    for (uint32_t ncat : {1u, 3u, 16u})
    for (uint32_t ncand : {1u, 2u, 12u})
    for (int derivs = 0; derivs < 2; ++derivs)
    for (int full = 0; full < 2; ++full) {
        const bool plain = mode == PGM_TREELIK_CALL_PLAIN, rates = mode == PGM_TREELIK_CALL_RATES, anc = mode == PGM_TREELIK_CALL_ANC, nni = mode == PGM_TREELIK_CALL_NNI;
        if ((plain && ncat != 1) || (!nni && ncand != 1) || (!(plain || rates) && derivs) || (!anc && full)) continue;   // (arguments the mode does not have)
        const PgmTreelikPlan p = pgm_treelik_plan(mode, dim, nleaves, nnodes, ncols, plain ? 0 : ncat, derivs != 0, nni ? ncand : 0, full != 0);
        ++plans;
        auto bad = [&](const char *what, const char *name) {
            ++findings;
            std::printf("mode %d dim %u nleaves %u nnodes %u ncols %u ncat %u ncand %u derivs %d full %d: %s: %s\n", mode, dim, nleaves, nnodes, ncols, ncat, ncand, derivs, full, name, what);
        };
        // what every region holds, in bytes
        const size_t nedges = nnodes - 1, ninner = nnodes - nleaves, C = plain ? 1 : ncat, X = derivs ? 3 : 1, nchunks = (ncols + 15) / 16;
        const size_t u = 8 * C * ninner * ncols * dim, cl = plain ? 0 : (size_t)ncat * ncols, ge = derivs ? 8 * nedges * ncols : 0;
        size_t want[PGM_TL_NREGIONS] = {};
        want[PGM_TL_CHILD] = 4 * (nnodes + 1 + nedges); want[PGM_TL_PI] = 8 * dim; want[PGM_TL_W] = plain ? 0 : 8 * ncat;
        want[PGM_TL_PARENT] = nni ? 4 * nnodes : 0; want[PGM_TL_CAND] = nni ? 12 * ncand : 0; want[PGM_TL_ROWS] = (size_t)nleaves * ncols;
        want[PGM_TL_P] = 8 * C * nedges * X * dim * dim;
        want[PGM_TL_U] = u; want[PGM_TL_O] = derivs || anc || nni ? u : 0;
        want[PGM_TL_CL] = 8 * cl; want[PGM_TL_CK] = 4 * cl; want[PGM_TL_GC] = want[PGM_TL_QC] = rates ? ge * ncat : 0;
        want[PGM_TL_G] = want[PGM_TL_H] = ge; want[PGM_TL_PART] = derivs ? 8 * 2 * nedges * nchunks : 0;
        want[PGM_TL_SITE_L] = 8 * ncols; want[PGM_TL_SITE_K] = 4 * ncols; want[PGM_TL_POST] = 8 * cl;
        want[PGM_TL_D1] = want[PGM_TL_D2] = derivs ? 8 * nedges : 0;
        want[PGM_TL_ANC_PROB] = anc ? 8 * ninner * ncols : 0; want[PGM_TL_ANC_STATE] = anc ? ninner * ncols : 0; want[PGM_TL_ANC_POST] = anc && full ? 8 * ninner * ncols * dim : 0;
        want[PGM_TL_RHO] = nni ? 8 * (size_t)ncand * ncols : 0;

        size_t end[PGM_TL_NSLOTS] = {};
        for (const Kind &k : kKinds) {
            const PgmTreelikRegion &r = p.r[k.region];
            if (r.bytes != want[k.region]) bad("not the size of its contents", k.name);
            if (r.bytes == 0) continue;
            if ((int)r.slot != k.slot) bad("in another slot", k.name);
            if (r.off % k.align) bad("misaligned", k.name);
            if (r.off + r.bytes > p.slot_bytes[k.slot]) bad("past the end of its slot", k.name);
            for (const Kind &o : kKinds) {
                const PgmTreelikRegion &q = p.r[o.region];
                if (o.region != k.region && q.bytes && q.slot == r.slot && q.off < r.off + r.bytes && r.off < q.off + q.bytes) bad("overlaps another region", k.name);
            }
            if (r.off + r.bytes > end[k.slot]) end[k.slot] = r.off + r.bytes;
        }
        for (int s = 0; s < PGM_TL_NSLOTS; ++s)
            if (p.slot_bytes[s] != end[s]) bad("does not end with its last region", kSlots[s]);
    }
    std::printf("%ld plans\n", plans);
    return findings || plans == 0 ? 1 : 0;
}
