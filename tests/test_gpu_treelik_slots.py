"""The five scratch slots the four tree likelihood entries share (csrc/pgm_treelik_plan.h) on the MI355X: on one context of its own
the entries are called in turn, so each finds the slots in the layout the one before left behind, over shapes that make the slots
grow, shrink and grow again; then once more with the entries in the opposite order and the two entries that have them without
derivatives, a further layout.  Every output is preset to garbage and compared bit for bit with the numpy statement (the check()
helpers of tests/test_gpu_ml*.py, the cases of their generators)."""
import pytest

import test_gpu_mlancestral as TA
import test_gpu_mlgamma as TR
import test_gpu_mlsearch as TN
import test_gpu_mltree as TO
import treelik_anc_ref as A
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R

pytestmark = pytest.mark.gpu

# (dim, ncols, tree, ncat, anc_post asked): tiny, the largest, small, medium
SHAPES = [(3, 1, "three", 1, False), (64, 17, "balanced8", 3, True), (64, 1, "three", 3, False), (3, 17, "balanced8", 1, True)]


def test_entries_in_turn_on_one_context():
    import prographmsa_amd as pg

    def plain(ctx, s, derivs):
        TO.check(ctx, R.make_case(s[0], s[1], s[2], derivs), ("plain", s, derivs))

    def rates(ctx, s, derivs):
        TR.check(ctx, G.make_case(s[0], s[1], s[2], s[3], derivs), ("rates", s, derivs))

    def ancestral(ctx, s, derivs):
        TA.check(ctx, A.make_case(s[0], s[1], s[2], s[3]), ("ancestral", s), full=s[4])

    def nni(ctx, s, derivs):
        case = N.make_case(s[0], s[1], s[2], s[3])
        assert len(case["cand"]) == {"three": 2, "balanced8": 12}[s[2]]   # every candidate the tree has
        TN.check(ctx, case, ("nni", s))

    entries = [plain, rates, ancestral, nni]
    own = pg.Context(0)
    try:
        for order, derivs in ((entries, True), (entries[::-1], False)):
            for s in SHAPES:
                for entry in order:
                    entry(own, s, derivs)
    finally:
        own.close()
