"""pgm_tree_nni on the MI355X against tests/treelik_nni_ref.py: equality of site_l, site_k, post and rho bit for bit, every output preset
to garbage; then `pgmsa --ml_tree --ml_search --stats` against pgmsa_oracle byte for byte.

The cases (tests/test_cpu_mlsearch.py holds the lists; its stand-alone host program runs the same ones): every dim of {4, 20, 61, 64}
with ncols of {1, 15, 16, 17, 33} and ncat of {1, 2, 4} on the balanced tree of 8 leaves with all 12 candidates (a workgroup of the
candidates' kernel holds 4 x 64 / dim sites: one site per wavefront at 61 and 64 states, 16 per wavefront at 4, so 15 .. 17 and 33
columns sit on both sides of a wavefront's and of a workgroup's edge); the trees of 3 leaves (2 candidates) and 4 leaves (the
candidates at the root's edges); the trifurcating root and an inner trifurcation; 24 leaves; the caterpillar of 96 leaves, where the
two trees of a candidate rescale a different number of times; a single candidate; candidates shuffled and repeated; 70001 candidates (more than the grid's second dimension); leaves with a
state, a gap and -2 as a and c, columns of gaps.  The expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mlsearch as TS
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R

pytestmark = pytest.mark.gpu

GARBAGE_F, GARBAGE_I = -7.25e77, -77777


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncat, ncols, ncand):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full((ncand, ncols), GARBAGE_F))


def check(ctx, case, what):
    ncols = case["rows"].shape[1]
    out = ctx.tree_nni(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["cand"], out=garbage(case["ncat"], ncols, len(case["cand"])))
    want = case["want"]
    assert not np.any(np.isnan(want["site_l"])) and not np.any(np.isnan(want["post"])) and not np.any(np.isnan(want["rho"]))
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    assert R.same_bits(out[2], want["post"]), what
    assert R.same_bits(out[3], want["rho"]), what
    return out


@pytest.mark.parametrize("key", TS.GRID)
def test_balanced_tree_of_8(ctx, key):
    case = N.make_case(*key)
    assert len(case["cand"]) == 12
    check(ctx, case, key)


@pytest.mark.parametrize("key", TS.SMALL_TREES + TS.ARITY)
def test_small_trees_and_other_arities(ctx, key):
    case = N.make_case(*key)
    if key[2] == "three":
        assert len(case["cand"]) == 2
    if key[2] == "four":
        assert len(case["cand"]) == 4 and all(int(case["parent"][int(v)]) == len(case["parent"]) - 1 for v in case["cand"][:, 0])
    check(ctx, case, key)


@pytest.mark.parametrize("key", TS.LARGER)
def test_larger_trees(ctx, key):
    case = N.make_case(*key)
    out = check(ctx, case, key)
    if key[2] == "caterpillar96":
        want = case["want"]
        assert (want["cat_kd"] != want["cat_kn"]).any()   # the scaling case: the two trees of a candidate count differently
        assert np.all(np.isfinite(out[3])) and np.all(out[3] > 0)


@pytest.mark.parametrize("key", TS.ORDER)
def test_one_candidate_and_candidates_in_any_order(ctx, key):
    case = N.make_case(*key)
    if key[4] == "one":
        assert len(case["cand"]) == 1
    else:
        assert len({tuple(c) for c in case["cand"].tolist()}) == len(case["cand"]) - 3
    check(ctx, case, key)


def test_leaves_as_a_and_c_and_columns_of_gaps(ctx):
    case = TS.leaf_case()
    assert (case["rows"][:, 4] == -1).all() and (case["rows"][:, 7] == -1).all()
    check(ctx, case, "leaves")


def test_more_candidates_than_the_grid_holds(ctx):
    """70001 candidates: the launch has 65535 workgroups along the candidates and 4466 of them take a second one."""
    case = TS.many_candidates_case()
    assert len(case["cand"]) == 70001 > 65535 and not R.same_bits(case["want"]["rho"][0], case["want"]["rho"][1])
    check(ctx, case, "70001 candidates")


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 4), (20, 17, "balanced8", 2), (61, 15, "balanced8", 2), (64, 33, "balanced8", 4)])
def test_site_values_equal_the_rates_entry(ctx, key):
    case = N.make_case(*key)
    nedges, ncols, ncat = len(case["parent"]) - 1, case["rows"].shape[1], case["ncat"]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood_rates(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=False,
                                    out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and R.same_bits(new[2], old[2])


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 1), (20, 17, "balanced8", 1), (61, 16, "balanced8", 1), (64, 15, "balanced8", 1)])
def test_one_category_equals_the_plain_entry(ctx, key):
    case = N.make_case(*key)
    assert case["w"].tolist() == [1.0]
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood(case["dim"], case["parent"], case["rows"], case["pi"], case["P"], derivs=False,
                              out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and np.all(new[2] == 1.0)
    assert R.same_bits(new[3], case["want"]["cat_rho"][0])   # (1.0 * x and 0.0 + x are exact)


def test_calls_of_different_shapes_on_one_context(ctx):
    """Large, small, large again, the older entries in between: nothing of a call is read by the next (the entries share their
    scratch buffers)."""
    import test_gpu_mlancestral as TA
    import test_gpu_mlgamma as TR
    import test_gpu_mltree as TO
    import treelik_anc_ref as A
    order = [("nni", (20, 33, "balanced24", 4)), ("rates", (20, 33, "balanced8", 4)), ("nni", (4, 1, "balanced8", 2)), ("old", (20, 300, "balanced8")), ("nni", (64, 33, "balanced8", 4)),
             ("anc", (4, 300, "balanced8", 4)), ("nni", (4, 17, "caterpillar96", 1)), ("nni", (4, 33, "balanced8", 4, "one")), ("anc", (20, 33, "balanced8", 16)),
             ("nni", (20, 33, "balanced24", 4))]
    for k, (which, key) in enumerate(order):
        what = ("call %d" % k,) + key
        if which == "nni":
            check(ctx, N.make_case(*key), what)
        elif which == "anc":
            TA.check(ctx, A.make_case(*key), what)
        elif which == "rates":
            TR.check(ctx, G.make_case(*key), what)
        else:
            TO.check(ctx, R.make_case(*key), what)


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = N.make_case(*TS.SMALL_VALID)
    parent, rows, pi, w, Pm = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["w"].copy(), case["P"].copy()
    cv, ca, cc = (np.ascontiguousarray(case["cand"][:, k]) for k in range(3))
    outs = garbage(2, 15, 12)
    f = pg.lib.pgm_tree_nni
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double), 12,
            P(cv, C.c_uint32), P(ca, C.c_uint32), P(cc, C.c_uint32), P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_double)]
    bad, keep = [], []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 4, 6, 7, 9, 10, 12, 13, 14, 15, 16, 17, 18):            # null pointers (the candidate arrays and rho among them)
        call({k: None})
    call({11: 0})                                                         # no candidate
    for k, v in ((8, 0), (8, 17), (8, 0xFFFFFFFF)):                       # ncat outside 1 .. 16
        call({k: v})
    for v in (0.0, -0.5, float("nan"), float("inf")):                     # a weight that is not finite and > 0
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
    for cand in TS.bad_candidates():                                      # a candidate that is none, alone or behind a good one
        arr = np.array(cand, np.uint32)
        cols = [np.ascontiguousarray(arr[:, k]) for k in range(3)]
        keep.append(cols)
        call({11: len(arr), 12: P(cols[0], C.c_uint32), 13: P(cols[1], C.c_uint32), 14: P(cols[2], C.c_uint32)})
    for at in (0, 5, 11):                                                 # ... and as one of the twelve
        cols = [cv.copy(), ca.copy(), cc.copy()]
        cols[2][at] = cols[0][at]                                        # c == v
        keep.append(cols)
        call({12: P(cols[0], C.c_uint32), 13: P(cols[1], C.c_uint32), 14: P(cols[2], C.c_uint32)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(outs[0] == GARBAGE_F) and np.all(outs[1] == GARBAGE_I) and np.all(outs[2] == GARBAGE_F) and np.all(outs[3] == GARBAGE_F)
    # the context is as good as before
    assert f(*args) == 0
    want = case["want"]
    assert R.same_bits(outs[0], want["site_l"]) and np.array_equal(outs[1], want["site_k"]) and R.same_bits(outs[2], want["post"]) and R.same_bits(outs[3], want["rho"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0
    for wrong in (dict(pi=pi[:3]), dict(P=Pm[:-1]), dict(w=w.reshape(1, 2)), dict(cand=case["cand"][:, :2])):   # the binding's own checks
        kw = dict(pi=pi, w=w, P=Pm, cand=case["cand"]); kw.update(wrong)
        with pytest.raises(ValueError):
            ctx.tree_nni(4, parent, rows, kw["pi"], kw["w"], kw["P"], kw["cand"])
    with pytest.raises(ValueError):
        ctx.tree_nni(4, parent, rows, pi, w, Pm, case["cand"], out=outs[:3] + (np.zeros((11, 15)),))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


fams = TS.fams


@pytest.mark.parametrize("start", ["one", "two", "swapped_pairs"])
@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"]])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, start, opts):
    """The 8-taxon search fixtures with the device switch: the tree, the sites file, the log and ml_lnl of the product driver are the
    oracle driver's (the host loop), byte for byte."""
    opts = TS.DNA(fams) + opts
    env = dict(os.environ, PGM_DEVICE_TREELIK="1")
    got = TS.run_s(exe, fams["sim8"], tmp_path, "hip", opts, search=10, start=fams[start], env=env)
    ref = TS.run_s(os.path.join(oracle_build, "pgmsa_oracle"), fams["sim8"], tmp_path, "ref", opts, search=10, start=fams[start])
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert (got.tree, got.sites, got.log_text, got.stdout) == (ref.tree, ref.sites, ref.log_text, ref.stdout)
    assert got.stats["ml_lnl"] == ref.stats["ml_lnl"] and got.stats["ml_lnl_start"] == ref.stats["ml_lnl_start"]
    for k in ("ml_search_rounds", "ml_nni_applied", "ml_nni_calls", "ml_rounds", "ml_evaluations"):
        assert got.stats[k] == ref.stats[k], k
    assert len(got.log) >= 2 and N.bipartitions(got.tree) == N.bipartitions(TS.TRUE8)
    assert got.stats["ml_nni_kernel_ms"] > 0 and got.stats["ml_kernel_ms"] > 0 and ref.stats["ml_nni_kernel_ms"] == 0
    assert "PGM_DEVICE_TREELIK" in got.stats["switches"]


def test_default_route_by_size(exe, oracle_build, fams, tmp_path_factory, tmp_path):
    """8 taxa take the host loop by default and 24 the device; PGM_HOST_TREELIK keeps the host loop at 24: the same files either way."""
    d = tmp_path_factory.mktemp("mls_route")
    aa24 = [f for f in bu.aa_families(d) if f.endswith("_n24.fa")][0]
    got = TS.run_s(exe, aa24, tmp_path, "hip", search=2)
    ref = TS.run_s(os.path.join(oracle_build, "pgmsa_oracle"), aa24, tmp_path, "ref", search=2)
    host = TS.run_s(exe, aa24, tmp_path, "host", search=2, env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (got.tree, got.sites, got.log_text) == (ref.tree, ref.sites, ref.log_text) == (host.tree, host.sites, host.log_text)
    assert got.stats["ml_nni_kernel_ms"] > 0 and host.stats["ml_nni_kernel_ms"] == 0 and got.stats["ml_nni_calls"] >= 1
    small = TS.run_s(exe, fams["sim8"], tmp_path, "small", TS.DNA(fams), search=10, start=fams["one"])
    assert small.stats["ml_nni_kernel_ms"] == 0 and small.stats["ml_kernel_ms"] == 0 and small.stats["ml_nni_calls"] >= 2
