"""pgm_tree_spr on the MI355X against tests/treelik_spr_ref.py: equality of site_l, site_k, post and rho bit for bit, every output preset
to garbage; then `pgmsa --ml_tree --ml_search --ml_spr --stats` against pgmsa_oracle byte for byte.

The cases (tests/test_cpu_mlspr.py holds the lists; its stand-alone host program runs the same ones): every dim of {4, 20, 61, 64} with
ncols of {1, 15, 16, 17, 33} and ncat of {1, 2, 4} on the balanced tree of 8 leaves with all 124 valid candidates (a workgroup holds
4 x 64 / dim sites: 15 .. 17 and 33 columns sit on both sides of a wavefront's and of a workgroup's edge); dims {1, 2, 3, 5, 33, 63} at
1, spb, spb + 1 and 4 spb + 1 columns (spb = 64 / dim); the trees of 3 and 4 leaves, both roots with three children, the inner
trifurcation, 24 leaves at radius 3; the caterpillar of 96 at path lengths 1, 2, 15 and 16, where the two chains of a candidate
rescale a different number of times; 1025 columns; 70001 candidates; a single candidate; candidates shuffled and repeated; leaves with
a state, a gap and -2 as v and as y, columns of gaps; D == 0.  The expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mlsearch as TS
import test_cpu_mlspr as TP
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
import treelik_spr_ref as S

pytestmark = pytest.mark.gpu

GARBAGE_F, GARBAGE_I = -7.25e77, -77777


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncat, ncols, ncand):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full((ncand, ncols), GARBAGE_F))


def check(ctx, case, what):
    ncols = case["rows"].shape[1]
    out = ctx.tree_spr(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["Ph"], case["cand"],
                       out=garbage(case["ncat"], ncols, len(case["cand"])))
    want = case["want"]
    assert not np.any(np.isnan(want["site_l"])) and not np.any(np.isnan(want["post"])) and not np.any(np.isnan(want["rho"]))
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    assert R.same_bits(out[2], want["post"]), what
    assert R.same_bits(out[3], want["rho"]), what
    return out


@pytest.mark.parametrize("key", TP.GRID)
def test_balanced_tree_of_8(ctx, key):
    case = S.make_case(*key)
    assert len(case["cand"]) == 124
    check(ctx, case, key)


@pytest.mark.parametrize("key", TP.ODD_DIMS)
def test_other_dims_at_the_edges_of_a_wavefront(ctx, key):
    check(ctx, S.make_case(*key), key)


@pytest.mark.parametrize("key", TP.TREES + TP.WIDE)
def test_other_trees_and_many_columns(ctx, key):
    case = S.make_case(*key)
    if key[2] == "three":
        assert case["cand"].tolist() == [[0, 2], [1, 2]]   # the target lies beyond the root
    if key[2] == "balanced24":
        lens = [len(p[0]) - 1 + len(p[1]) for p in (S.path_of(case["parent"], int(v), int(y)) for v, y in case["cand"])]
        assert max(lens) == 3 and len(lens) > 200
    check(ctx, case, key)


@pytest.mark.parametrize("dim,ncat", [(4, 1), (20, 2)])
def test_caterpillar_paths_and_scaling(ctx, dim, ncat):
    case = TP.caterpillar_case(dim, ncat)
    lens = {len(p[0]) - 1 + len(p[1]) for p in (S.path_of(case["parent"], int(v), int(y)) for v, y in case["cand"])}
    assert lens == {1, 2, 15, 16}
    out = check(ctx, case, ("caterpillar", dim, ncat))
    want = case["want"]
    assert (want["cat_km"] != want["cat_kp"]).any()   # the scaling case: the two chains of a candidate count differently
    assert np.all(np.isfinite(out[3])) and np.all(out[3] > 0)


def test_the_longest_path(ctx):
    case = TP.long_path_case(0)[0]
    case = dict(case, want=S.evaluate(2, 96, case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["Ph"], case["cand"]))
    check(ctx, case, "16 edges upward")


@pytest.mark.parametrize("key", TP.ORDER)
def test_one_candidate_and_candidates_in_any_order(ctx, key):
    case = S.make_case(*key)
    if key[4] == "one":
        assert len(case["cand"]) == 1
    else:
        assert len({tuple(c) for c in case["cand"].tolist()}) == len(case["cand"]) - 3
    check(ctx, case, key)


def test_leaves_as_v_and_y_and_columns_of_gaps(ctx):
    case = TP.leaf_case()
    assert (case["rows"][:, 4] == -1).all() and (case["rows"][:, 7] == -1).all()
    check(ctx, case, "leaves")


def test_zero_denominator(ctx):
    case = TP.zeros_case()
    assert (case["want"]["cat_l"][0] == 0.0).any()
    out = check(ctx, case, "zeros")
    assert np.all(np.isfinite(out[3]))


def test_more_candidates_than_the_grid_holds(ctx):
    """70001 candidates: the launch has 65535 workgroups along the candidates and 4466 of them take a second one."""
    case = TP.many_candidates_case()
    assert len(case["cand"]) == 70001 > 65535 and not R.same_bits(case["want"]["rho"][0], case["want"]["rho"][1])
    check(ctx, case, "70001 candidates")


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 4), (20, 17, "balanced8", 2), (61, 15, "balanced8", 2), (64, 33, "balanced8", 4)])
def test_site_values_equal_the_rates_entry(ctx, key):
    case = S.make_case(*key)
    nedges, ncols, ncat = len(case["parent"]) - 1, case["rows"].shape[1], case["ncat"]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood_rates(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=False,
                                    out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and R.same_bits(new[2], old[2])


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 1), (20, 17, "balanced8", 1), (61, 16, "balanced8", 1), (64, 15, "balanced8", 1)])
def test_one_category_equals_the_plain_entry(ctx, key):
    case = S.make_case(*key)
    assert case["w"].tolist() == [1.0]
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood(case["dim"], case["parent"], case["rows"], case["pi"], case["P"], derivs=False,
                              out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and np.all(new[2] == 1.0)
    assert R.same_bits(new[3], case["want"]["cat_rho"][0])   # (1.0 * x and 0.0 + x are exact)


def test_calls_interleaved_with_the_other_entries(ctx):
    """Large, small, large again, the other five entries in between: nothing of a call is read by the next (the entries share their
    scratch slots)."""
    import test_gpu_mlancestral as TA
    import test_gpu_mlgamma as TR
    import test_gpu_mlnniopt as TE
    import test_gpu_mlsearch as TN
    import test_gpu_mltree as TO
    import treelik_anc_ref as A
    import treelik_nni_edge_ref as E
    order = [("spr", (20, 33, "balanced24", 4, "all", 3)), ("rates", (20, 33, "balanced8", 4)), ("spr", (4, 1, "balanced8", 2)), ("old", (20, 300, "balanced8")),
             ("spr", (64, 33, "balanced8", 4)), ("nni", (20, 33, "balanced24", 4)), ("spr", (4, 33, "balanced8", 4, "one")), ("anc", (4, 300, "balanced8", 4)),
             ("spr", (4, 17, "three", 2)), ("edge", None), ("spr", (20, 33, "balanced24", 4, "all", 3))]
    for k, (which, key) in enumerate(order):
        what = ("call %d" % k,) + (key or ())
        if which == "spr":
            check(ctx, S.make_case(*key), what)
        elif which == "nni":
            TN.check(ctx, N.make_case(*key), what)
        elif which == "anc":
            TA.check(ctx, A.make_case(*key), what)
        elif which == "rates":
            TR.check(ctx, G.make_case(*key), what)
        elif which == "edge":
            edge_call(ctx, TE, E)
        else:
            TO.check(ctx, R.make_case(*key), what)
    check(ctx, TP.caterpillar_case(4, 1), "caterpillar, last")


def edge_call(ctx, TE, E):
    """One pgm_tree_nni_edge call between two pgm_tree_spr calls, checked as tests/test_gpu_mlnniopt.py checks its own."""
    case = E.make_case(4, 17, "balanced8", 2)
    TE.check(ctx, case, "edge between spr calls")


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = S.make_case(*TP.SMALL_VALID)
    parent, rows, pi, w, Pm, Ph = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["w"].copy(), case["P"].copy(), case["Ph"].copy()
    cv, cy = (np.ascontiguousarray(case["cand"][:, k]) for k in range(2))
    ncand = len(cv)
    outs = garbage(2, 15, ncand)
    f = pg.lib.pgm_tree_spr
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double), P(Ph, C.c_double), ncand,
            P(cv, C.c_uint32), P(cy, C.c_uint32), P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_double)]
    bad, keep = [], []

    def call(changes, a=None):
        a = list(args if a is None else a)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 4, 6, 7, 9, 10, 11, 13, 14, 15, 16, 17, 18):            # null pointers (Ph, the candidate arrays and rho among them)
        call({k: None})
    call({12: 0})                                                         # no candidate
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
    for cand in TP.bad_candidates():                                      # a candidate that is none, alone or behind a good one
        arr = np.array(cand, np.uint32)
        cols = [np.ascontiguousarray(arr[:, k]) for k in range(2)]
        keep.append(cols)
        call({12: len(arr), 13: P(cols[0], C.c_uint32), 14: P(cols[1], C.c_uint32)})
    for at in (0, 60, ncand - 1):                                         # ... and as one of the 124
        cols = [cv.copy(), cy.copy()]
        cols[1][at] = cols[0][at]                                        # y == v
        keep.append(cols)
        call({13: P(cols[0], C.c_uint32), 14: P(cols[1], C.c_uint32)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    # a path of 17 edges on the caterpillar: refused, and the same outputs stay untouched (one column, one candidate)
    longer, _ = TP.long_path_case(1)
    lp, lr, lpi, lw, lP, lH = (np.ascontiguousarray(longer[k]) for k in ("parent", "rows", "pi", "w", "P", "Ph"))
    lv, ly = (np.ascontiguousarray(longer["cand"][:, k]) for k in range(2))
    rc = f(ctx.handle, 2, 96, len(lp), P(lp, C.c_uint32), 1, P(lr, C.c_int8), P(lpi, C.c_double), 2, P(lw, C.c_double), P(lP, C.c_double), P(lH, C.c_double), 1,
           P(lv, C.c_uint32), P(ly, C.c_uint32), P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_double))
    assert rc == pg.PGM_ERR_INVALID and b"more than 16 edges" in pg.lib.pgm_last_error()
    assert np.all(outs[0] == GARBAGE_F) and np.all(outs[1] == GARBAGE_I) and np.all(outs[2] == GARBAGE_F) and np.all(outs[3] == GARBAGE_F)
    # the context is as good as before
    assert f(*args) == 0
    want = case["want"]
    assert R.same_bits(outs[0], want["site_l"]) and np.array_equal(outs[1], want["site_k"]) and R.same_bits(outs[2], want["post"]) and R.same_bits(outs[3], want["rho"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0
    for wrong in (dict(pi=pi[:3]), dict(P=Pm[:-1]), dict(Ph=Ph[:-1]), dict(w=w.reshape(1, 2)), dict(cand=np.zeros((3, 3), np.uint32))):   # the binding's own checks
        kw = dict(pi=pi, w=w, P=Pm, Ph=Ph, cand=case["cand"]); kw.update(wrong)
        with pytest.raises(ValueError):
            ctx.tree_spr(4, parent, rows, kw["pi"], kw["w"], kw["P"], kw["Ph"], kw["cand"])
    with pytest.raises(ValueError):
        ctx.tree_spr(4, parent, rows, pi, w, Pm, Ph, case["cand"], out=outs[:3] + (np.zeros((11, 15)),))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


fams = TP.fams


@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"]], ids=["one rate", "gamma4"])
@pytest.mark.parametrize("fam,start", [("spr8", "spr_start"), ("sim8", "swapped_pairs")])
def test_search_with_the_scan_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, fam, start, opts):
    """The CPU fixtures with the device switch: the tree, the sites file, the log and ml_lnl of the product driver are the oracle
    driver's (the host loop), byte for byte."""
    opts = TS.DNA(fams) + opts + ["--ml_spr", "4"]
    env = dict(os.environ, PGM_DEVICE_TREELIK="1")
    got = TS.run_s(exe, fams[fam], tmp_path, "hip", opts, search=20, start=fams[start], env=env)
    ref = TS.run_s(os.path.join(oracle_build, "pgmsa_oracle"), fams[fam], tmp_path, "ref", opts, search=20, start=fams[start])
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert (got.tree, got.sites, got.log_text, got.stdout) == (ref.tree, ref.sites, ref.log_text, ref.stdout)
    assert got.stats["ml_lnl"] == ref.stats["ml_lnl"] and got.stats["ml_lnl_start"] == ref.stats["ml_lnl_start"]
    for k in ("ml_search_rounds", "ml_nni_applied", "ml_nni_calls", "ml_spr_calls", "ml_spr_candidates", "ml_spr_applied", "ml_rounds", "ml_evaluations"):
        assert got.stats[k] == ref.stats[k], k
    assert any(line[8] == "spr" for line in got.log) and got.stats["ml_spr_calls"] >= 1
    assert got.stats["ml_spr_kernel_ms"] > 0 and ref.stats["ml_spr_kernel_ms"] == 0
    if fam == "spr8" and not opts.count("--ml_gamma"):
        assert N.bipartitions(got.tree) == N.bipartitions(TP.TRUE8) and got.stats["ml_spr_applied"] >= 1


def test_default_route_by_size(exe, oracle_build, fams, tmp_path_factory, tmp_path):
    """8 taxa take the host loop by default and 24 the device; PGM_HOST_TREELIK keeps the host loop at 24: the same files either way."""
    d = tmp_path_factory.mktemp("spr_route")
    aa24 = [f for f in bu.aa_families(d) if f.endswith("_n24.fa")][0]
    spr = ["--ml_spr", "2"]
    got = TS.run_s(exe, aa24, tmp_path, "hip", spr, search=2)
    ref = TS.run_s(os.path.join(oracle_build, "pgmsa_oracle"), aa24, tmp_path, "ref", spr, search=2)
    host = TS.run_s(exe, aa24, tmp_path, "host", spr, search=2, env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (got.tree, got.sites, got.log_text) == (ref.tree, ref.sites, ref.log_text) == (host.tree, host.sites, host.log_text)
    assert got.stats["ml_spr_calls"] >= 1 and got.stats["ml_spr_kernel_ms"] > 0   # (the interchanges stall within two rounds: the scan runs on the device)
    assert any(line[8] == "spr" for line in got.log)
    assert host.stats["ml_spr_kernel_ms"] == 0 and got.stats["ml_spr_calls"] == host.stats["ml_spr_calls"] == ref.stats["ml_spr_calls"]
    small = TS.run_s(exe, fams["spr8"], tmp_path, "small", TS.DNA(fams) + ["--ml_spr", "4"], search=20, start=fams["spr_start"])
    assert small.stats["ml_spr_kernel_ms"] == 0 and small.stats["ml_kernel_ms"] == 0 and small.stats["ml_spr_calls"] >= 2
