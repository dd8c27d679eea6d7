"""pgm_tree_ancestral on the MI355X against tests/treelik_anc_ref.py: equality of site_l, site_k, post, anc_state, anc_prob and anc_post
bit for bit, every output preset to garbage; then `pgmsa --ml_tree --ml_ancestral --stats` against pgmsa_oracle byte for byte.

The cases: every dim of {4, 20, 61, 64} with ncat of {1, 2, 4, 16} and ncols of {1, 17, 33} on the balanced tree of 8 leaves (one and
several workgroups of the walk, a partly filled wavefront: 61 states leave three lanes idle, 17 columns of 4 states fill a quarter of
the second workgroup); ncat = 4 and 33 columns on the trees of 2 leaves (the root alone), 3 and 24 leaves and the trifurcating root;
300 columns of 4 states (132 workgroups of the combine kernel over the node x site range); a caterpillar of 96 leaves whose two
categories rescale a different number of times (to a tiny posterior share, and to an exact 0.0); unequal weights; a tie of two
states; a category whose likelihood is 0.0.  The expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mlancestral as TA
import treelik_anc_ref as A
import treelik_rates_ref as G
import treelik_ref as R

pytestmark = pytest.mark.gpu

GARBAGE_F, GARBAGE_I, GARBAGE_B = -7.25e77, -77777, -99


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncat, ncols, ninner, dim):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full((ninner, ncols), GARBAGE_B, np.int8),
            np.full((ninner, ncols), GARBAGE_F), np.full((ninner, ncols, dim), GARBAGE_F))


def check(ctx, case, what, full=True):
    ninner, ncols = len(case["parent"]) - case["nleaves"], case["rows"].shape[1]
    out = ctx.tree_ancestral(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], full=full, out=garbage(case["ncat"], ncols, ninner, case["dim"]))
    want = case["want"]
    assert not np.any(np.isnan(want["site_l"])) and not np.any(np.isnan(want["post"])) and not np.any(np.isnan(want["anc_post"]))
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    assert R.same_bits(out[2], want["post"]), what
    assert np.array_equal(out[3], want["anc_state"]), what
    assert R.same_bits(out[4], want["anc_prob"]), what
    if full:
        assert R.same_bits(out[5], want["anc_post"]), what
    else:
        assert np.all(out[5] == GARBAGE_F), what   # untouched
    return out


# (the lists of cases live in tests/test_cpu_mlancestral.py: its stand-alone host program runs the same ones)
@pytest.mark.parametrize("key", TA.GRID)
def test_balanced_tree_of_8(ctx, key):
    check(ctx, A.make_case(*key), key)


@pytest.mark.parametrize("key", TA.OTHER_TREES)
def test_other_trees(ctx, key):
    check(ctx, A.make_case(*key), key)


def test_more_than_one_workgroup_of_the_combine_kernel(ctx):
    check(ctx, A.make_case(*TA.MANY_COLUMNS), "300 columns")


def test_mixed_scaling(ctx):
    """k_0 > k_1 on the columns without gaps: category 0's share of the mixture is tiny but the statement's."""
    case = A.make_mixed_scaling_case(*TA.MIXED_SCALING[0])
    out = check(ctx, case, "mixed scaling")
    hit = case["full"] & (case["diff"] >= 1)
    assert hit.any() and np.all(out[2][0][hit] > 0) and np.all(out[2][0][hit] < 1e-60)


@pytest.mark.parametrize("key", TA.MIXED_SCALING[1:])
def test_mixed_scaling_to_an_exact_zero(ctx, key):
    """Five shifts and more: post_0 is an exact 0.0 and the mixture is category 1's vector, bit for bit."""
    case = A.make_mixed_scaling_case(*key)
    out = check(ctx, case, "mixed scaling, five shifts and more")
    hit = case["full"] & (case["diff"] >= 5)
    assert hit.any() and np.all(out[2][0][hit] == 0.0) and np.all(out[2][1][hit] == 1.0)
    assert R.same_bits(out[5][:, hit, :], case["want"]["cat_a"][1][:, hit, :])


def test_unequal_weights(ctx):
    case = A.make_case(*TA.UNEQUAL)
    assert case["w"].tolist() == [0.1, 0.2, 0.3, 0.4]
    out = check(ctx, case, "unequal weights")
    assert not R.same_bits(out[5], A.make_case(4, 33, "balanced8", 4)["want"]["anc_post"])


def test_ties_and_a_category_of_likelihood_zero(ctx):
    out = check(ctx, TA.with_want(TA.tie_case()), "tie")
    assert np.all(out[3] == 1) and np.all(out[4] == 0.375)
    case = TA.with_want(TA.zero_case())
    out = check(ctx, case, "zero")
    assert np.all(out[2][0][[0, 2]] == 0.0) and np.all(out[3] >= 0)
    # category 0 alone: site_l and every Z are 0.0 at columns 0 and 2, post is 0 / 0 there and the node has no state
    ninner, ncols = 1, 4
    one = ctx.tree_ancestral(4, case["parent"], case["rows"], case["pi"], np.array([1.0]), case["P"][:32], out=garbage(1, ncols, ninner, 4))
    want = A.evaluate(4, 2, case["parent"], case["rows"], case["pi"], np.array([1.0]), case["P"][:32])
    assert R.same_bits(one[0], want["site_l"]) and np.array_equal(one[3], want["anc_state"]) and R.same_bits(one[4], want["anc_prob"])
    assert one[3][0].tolist()[0] == -1 and one[3][0].tolist()[2] == -1 and one[4][0, 0] == 0.0 and np.all(np.isnan(one[5][0, 0]))


@pytest.mark.parametrize("key", TA.NOT_FULL)
def test_without_the_full_posteriors(ctx, key):
    check(ctx, A.make_case(*key), key + ("full=False",), full=False)


@pytest.mark.parametrize("key", TA.ONE_CATEGORY)
def test_one_category_equals_the_rates_entry(ctx, key):
    case = A.make_case(*key)
    assert case["w"].tolist() == [1.0]
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood_rates(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=False,
                                    out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((1, ncols), GARBAGE_F), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and R.same_bits(new[2], old[2])
    assert R.same_bits(new[5], case["want"]["cat_a"][0])


def test_calls_of_different_shapes_on_one_context(ctx):
    """Large, small, large again, other numbers of categories, the two older entries in between: nothing of a call is read by the next
    (the three entries share their scratch buffers)."""
    import test_gpu_mlgamma as TR
    import test_gpu_mltree as TO
    order = [("anc", (20, 33, "balanced8", 16)), ("rates", (20, 33, "balanced8", 4)), ("anc", (4, 1, "balanced8", 2)), ("old", (20, 300, "balanced8")), ("anc", (64, 33, "balanced24", 4)),
             ("rates", (4, 300, "balanced8", 4)), ("anc", (4, 300, "balanced8", 4)), ("old", (64, 33, "balanced24")), ("anc", (4, 17, "balanced8", 1)), ("anc", (20, 33, "balanced8", 16))]
    assert all(key in TA.MIXED_SHAPES for which, key in order if which == "anc")
    for k, (which, key) in enumerate(order):
        what = ("call %d" % k,) + key
        if which == "anc":
            check(ctx, A.make_case(*key), what, full=k % 2 == 0)
        elif which == "rates":
            TR.check(ctx, G.make_case(*key), what)
        else:
            TO.check(ctx, R.make_case(*key), what)


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = A.make_case(*TA.SMALL_VALID)
    parent, rows, pi, w, Pm = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["w"].copy(), case["P"].copy()
    outs = garbage(2, 15, 7, 4)
    f = pg.lib.pgm_tree_ancestral
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double),
            P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_int8), P(outs[4], C.c_double), P(outs[5], C.c_double)]
    bad, keep = [], []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 4, 6, 7, 9, 10, 11, 12, 13, 14, 15):                    # null pointers (anc_state and anc_prob among them)
        call({k: None})
    for k, v in ((8, 0), (8, 17), (8, 0xFFFFFFFF)):                       # ncat outside 1 .. 16
        call({k: v})
    for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):      # a weight that is not finite and > 0
        ww = w.copy(); ww[1] = v; keep.append(ww)
        call({9: P(ww, C.c_double)})
    for k, v in ((1, 0), (1, 65), (2, 1), (2, 0), (5, 0), (3, 8), (3, 7)):   # what the likelihood entries refuse
        call({k: v})
    for changes in ({8: 8}, {8: 3}, {9: 15}, {0: 3}, {0: 9}, {13: 0xFFFFFFFF}):
        p = parent.copy()
        for k, v in changes.items():
            p[k] = v
        keep.append(p)
        call({4: P(p, C.c_uint32)})
    for v in (4, -3, 127, -128):
        r = rows.copy(); r[7, 14] = v; keep.append(r)
        call({6: P(r, C.c_int8)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(outs[0] == GARBAGE_F) and np.all(outs[1] == GARBAGE_I) and np.all(outs[2] == GARBAGE_F) and np.all(outs[3] == GARBAGE_B)
    assert np.all(outs[4] == GARBAGE_F) and np.all(outs[5] == GARBAGE_F)
    # anc_post may be null, and the context is as good as before
    a = list(args); a[16] = None
    assert f(*a) == 0
    want = case["want"]
    assert R.same_bits(outs[0], want["site_l"]) and np.array_equal(outs[3], want["anc_state"]) and R.same_bits(outs[4], want["anc_prob"]) and np.all(outs[5] == GARBAGE_F)
    assert f(*args) == 0
    assert R.same_bits(outs[5], want["anc_post"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0
    for wrong in (dict(pi=pi[:3]), dict(P=Pm[:-1]), dict(w=w.reshape(1, 2))):   # the binding's own checks
        kw = dict(pi=pi, w=w, P=Pm); kw.update(wrong)
        with pytest.raises(ValueError):
            ctx.tree_ancestral(4, parent, rows, kw["pi"], kw["w"], kw["P"])
    with pytest.raises(ValueError):
        ctx.tree_ancestral(4, parent, rows, pi, w, Pm, out=outs[:5] + (None,))   # full without a buffer for it


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mla_fams")
    aa = bu.aa_families(d)
    return dict(aa24=[f for f in aa if f.endswith("_n24.fa")][0], aa5=[f for f in aa if f.endswith("_n5.fa")][0])


@pytest.mark.parametrize("fam,env", [("aa24", {}), ("aa5", {"PGM_DEVICE_TREELIK": "1"})])
@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"]])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, fam, env, opts):
    """24 taxa take the device route by default, 5 with the switch: the three files, the other outputs and the stats of the product
    driver are the oracle driver's (the host loop), byte for byte."""
    opts = ["-i", "0"] + opts
    got = TA.run_a(exe, fams[fam], tmp_path, "hip", opts, env=dict(os.environ, **env))
    ref = TA.run_a(os.path.join(oracle_build, "pgmsa_oracle"), fams[fam], tmp_path, "ref", opts)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert (got.anc, got.anctree, got.probs) == (ref.anc, ref.anctree, ref.probs)
    assert (got.tree, got.sites, got.rates, got.stdout) == (ref.tree, ref.sites, ref.rates, ref.stdout)
    assert len(got.anc) > 0 and len(got.anctree) > 0 and len(got.probs) > 0
    assert got.stats["ml_kernel_ms"] > 0 and ref.stats["ml_kernel_ms"] == 0 and got.stats["ml_ancestral_s"] > 0
    assert ("PGM_DEVICE_TREELIK" in got.stats["switches"]) == bool(env)
    without = TA.run_a(exe, fams[fam], tmp_path, "without", opts, env=dict(os.environ, **env), anc=False, tree=False, probs=False)
    assert "ml_ancestral_s" not in without.stats and without.stats["ml_kernel_ms"] > 0
    host = TA.run_a(exe, fams[fam], tmp_path, "host", opts, env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (host.anc, host.anctree, host.probs) == (got.anc, got.anctree, got.probs) and host.stats["ml_kernel_ms"] == 0
