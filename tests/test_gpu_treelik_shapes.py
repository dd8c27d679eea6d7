"""The four tree likelihood entries on the MI355X at the shapes their own files leave out, against the numpy statements bit for bit, every
output preset to garbage (the check() helpers of tests/test_gpu_ml*.py).  tests/test_cpu_treelik_shapes.py holds the lists of cases and
says what each is for; its stand-alone host programs run the same ones, but for the two large cases of part B.

A. every kind of dim beside {4, 20, 61, 64}, at 1, spb, spb + 1 and 4 spb + 1 columns (spb = 64 / dim sites per wavefront);
B. the second round of the sums kernel's loop over chunks (more than 1024 columns), of the combine kernel's loop over edges (more than
   65535 edges) and of the ancestral combine kernel's loop over (node, site) pairs (more than 2^20 pairs);
C. polytomies below the root, a star, a root of mixed children.

Whoever changes one of those three launch caps moves the case of B that sits just past it (the test notes of 3.17 to 3.20)."""
import numpy as np
import pytest

import test_cpu_treelik_shapes as SH
import test_gpu_mlancestral as TA
import test_gpu_mlgamma as TR
import test_gpu_mlsearch as TN
import test_gpu_mltree as TO
import treelik_anc_ref as A
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R

pytestmark = pytest.mark.gpu


def _rescaled_on_full_columns(case, site_k):
    full = (case["rows"] >= 0).all(axis=0)
    assert full.any() and np.all(site_k[full] > 0)   # the scaling path ran


# ---- A: every kind of dim --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SH.DIMS_PLAIN, ids=SH.ident)
def test_plain_at_every_kind_of_dim(ctx, key):
    out = TO.check(ctx, R.make_case(*key), key)
    assert np.all(out[1] == 0)


@pytest.mark.parametrize("key", SH.DIMS_RATES, ids=SH.ident)
def test_rates_at_every_kind_of_dim(ctx, key):
    TR.check(ctx, G.make_case(*key), key)


@pytest.mark.parametrize("key", SH.DIMS_ANC, ids=SH.ident)
def test_ancestral_at_every_kind_of_dim(ctx, key):
    TA.check(ctx, A.make_case(*key), key, full=True)


@pytest.mark.parametrize("key", SH.DIMS_NNI, ids=SH.ident)
def test_nni_at_every_kind_of_dim(ctx, key):
    case = N.make_case(*key)
    assert len(case["cand"]) == 12
    TN.check(ctx, case, key)


@pytest.mark.parametrize("key", SH.SCALING_PLAIN, ids=SH.ident)
def test_plain_scaling_path(ctx, key):
    """The caterpillar of 96 leaves, every matrix entry in [0.03, 0.07]: every column without missing data rescales, at one state too."""
    case = R.make_case(*key)
    _rescaled_on_full_columns(case, TO.check(ctx, case, key)[1])


@pytest.mark.parametrize("key", SH.SCALING_RATES, ids=SH.ident)
def test_rates_scaling_path(ctx, key):
    case = G.make_case(*key)
    _rescaled_on_full_columns(case, TR.check(ctx, case, key)[1])


@pytest.mark.parametrize("key", SH.NO_DERIVS, ids=SH.ident)
def test_plain_without_derivatives(ctx, key):
    case = R.make_case(*key)
    assert not case["derivs"]
    TO.check(ctx, case, key)
    assert R.same_bits(case["want"]["site_l"], R.make_case(*key[:3])["want"]["site_l"])   # (the same up pass)


# ---- B: the second rounds of the strided loops ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SH.SUMS_PLAIN, ids=SH.ident)
def test_plain_more_chunks_than_threads_of_the_sums_kernel(ctx, key):
    """1024 columns are 64 chunks of 16, one per thread; 1025 give thread 0 a second chunk of one site, 2049 a third."""
    TO.check(ctx, R.make_case(*key), key)


@pytest.mark.parametrize("key", SH.SUMS_RATES, ids=SH.ident)
def test_rates_more_chunks_than_threads_of_the_sums_kernel(ctx, key):
    TR.check(ctx, G.make_case(*key), key)


def test_rates_more_edges_than_the_grid_holds(ctx):
    """65538 edges: the combine kernel's launch has 65535 workgroups along the edges and three of them take a second one.  check()
    compares site_l, site_k, post and every entry of d1 and d2."""
    case = SH.edges_case()
    nedges = len(case["parent"]) - 1
    assert nedges == 65538 > SH.EDGES_GRID and case["derivs"] and case["ncat"] == 2
    out = TR.check(ctx, case, "65538 edges")
    assert out[3].shape == (nedges,) and not np.any(out[3][SH.EDGES_GRID:] == TR.GARBAGE_F) and not np.any(out[4][SH.EDGES_GRID:] == TR.GARBAGE_F)
    assert np.all(out[1] > 0)   # (a tree this large rescales)


def test_ancestral_more_pairs_than_the_grid_holds():
    """2^20 + 3 (node, site) pairs at 33 states, one pair per wavefront: the ancestral combine kernel's launch has 2^20 workgroups and
    three of them take a second pair.  The expectation is that of 1021 columns repeated (tests/test_cpu_treelik_shapes.py:
    test_columns_are_independent).  Without anc_post; the call's scratch is some 1.1 GB, so it has a context of its own."""
    import prographmsa_amd as pg
    case = SH.pairs_case()
    ncols, want = case["rows"].shape[1], case["want"]
    assert ncols == SH.PAIRS_NCOLS and (len(case["parent"]) - case["nleaves"]) * ncols > SH.PAIRS_GRID
    out = (np.full(ncols, TA.GARBAGE_F), np.full(ncols, TA.GARBAGE_I, np.int32), np.full((2, ncols), TA.GARBAGE_F), np.full((1, ncols), TA.GARBAGE_B, np.int8),
           np.full((1, ncols), TA.GARBAGE_F), None)
    own = pg.Context(0)
    try:
        own.tree_ancestral(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], full=False, out=out)
    finally:
        own.close()
    assert not np.any(np.isnan(want["site_l"])) and not np.any(np.isnan(want["post"])) and not np.any(np.isnan(want["anc_prob"]))
    assert R.same_bits(out[0], want["site_l"]) and np.array_equal(out[1], want["site_k"]) and R.same_bits(out[2], want["post"])
    assert np.array_equal(out[3][:, SH.PAIRS_GRID:], want["anc_state"][:, SH.PAIRS_GRID:]) and R.same_bits(out[4][:, SH.PAIRS_GRID:], want["anc_prob"][:, SH.PAIRS_GRID:])   # the second round
    assert np.array_equal(out[3], want["anc_state"]) and R.same_bits(out[4], want["anc_prob"])
    assert np.all(want["anc_state"] >= 0) and np.all(want["anc_prob"] > 0)


# ---- C: polytomies ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SH.POLY_PLAIN, ids=SH.ident)
def test_plain_polytomies(ctx, key):
    out = TO.check(ctx, R.make_case(*key), key)
    assert np.all(out[1] == 0)


@pytest.mark.parametrize("key", SH.POLY_RATES, ids=SH.ident)
def test_rates_polytomies(ctx, key):
    TR.check(ctx, G.make_case(*key), key)


@pytest.mark.parametrize("key", SH.POLY_ANC, ids=SH.ident)
def test_ancestral_polytomies(ctx, key):
    TA.check(ctx, A.make_case(*key), key, full=True)


@pytest.mark.parametrize("key", SH.POLY_NNI, ids=SH.ident)
def test_nni_polytomies(ctx, key):
    case = N.make_case(*key)
    assert len(case["cand"]) == {"inner3": 7, "inner4": 16, "leaves4": 6, "mixed3": 10}[key[2]]   # every candidate the tree has
    TN.check(ctx, case, key)
