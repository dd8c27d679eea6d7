"""pgm_tree_nni_edge on the MI355X against tests/treelik_nni_edge_ref.py: equality of site_l, site_k, post, rho, d1 and d2 bit for bit,
every output preset to garbage; then `pgmsa --ml_nni_opt` against pgmsa_oracle byte for byte.

The cases (tests/test_cpu_mlnniopt.py holds the lists; its stand-alone host program runs the same ones): every dim of {4, 20, 61, 64}
with ncols of {1, 15, 16, 17, 33} and ncat of {1, 2, 4} on the balanced tree of 8 leaves with all 12 candidates; dims {1, 2, 3, 5, 33,
63} at 1, spb = 64 / dim, spb + 1, 4 spb and 4 spb + 1 columns (a wavefront's and a workgroup's sites, and one more); the trees of 3
and 4 leaves, the trifurcating root, the inner trifurcation, 24 leaves, the caterpillar of 96 with its scaling case; 1025 columns (65 chunks: the second
round of the sums kernel's chunk loop); 70001 candidates of 2 states on one column (the candidate stride loop's second round); a single
candidate, shuffled and repeated candidates, one candidate with eight sets of matrices; leaves, gaps and -2 as a and c, all-gap
columns; matrices with zeros (D == 0, rho == 0).  The expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mlnniopt as TE
import test_cpu_mlsearch as TS
import test_cpu_mlsupport as TSUP
import treelik_nni_edge_ref as E
import treelik_nni_ref as N
import treelik_ref as R

pytestmark = pytest.mark.gpu

GARBAGE_F, GARBAGE_I = -7.25e77, -77777


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncat, ncols, ncand):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full((ncand, ncols), GARBAGE_F),
            np.full(ncand, GARBAGE_F), np.full(ncand, GARBAGE_F))


def check(ctx, case, what):
    ncols = case["rows"].shape[1]
    out = ctx.tree_nni_edge(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["cand"], case["Pc"],
                            out=garbage(case["ncat"], ncols, len(case["cand"])))
    want = case["want"]
    assert not any(np.any(np.isnan(want[k])) for k in ("site_l", "post", "rho", "d1", "d2")), what
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    assert R.same_bits(out[2], want["post"]), what
    assert R.same_bits(out[3], want["rho"]), what
    assert R.same_bits(out[4], want["d1"]) and R.same_bits(out[5], want["d2"]), what
    return out


@pytest.mark.parametrize("key", TE.GRID)
def test_balanced_tree_of_8(ctx, key):
    case = E.make_case(*key)
    assert len(case["cand"]) == 12
    check(ctx, case, key)


@pytest.mark.parametrize("key", TE.OTHER_DIMS)
def test_other_dims_at_the_edges_of_a_workgroup(ctx, key):
    check(ctx, E.make_case(*key), key)


@pytest.mark.parametrize("key", TE.TREES + TE.ORDER + TE.LONG)
def test_trees_orders_and_many_columns(ctx, key):
    case = E.make_case(*key)
    out = check(ctx, case, key)
    if key[2] == "caterpillar96":
        nw = case["nni_want"]
        assert (nw["cat_kd"] != nw["cat_kn"]).any() and np.all(np.isfinite(out[3])) and np.all(out[3] > 0)
    if key in TE.LONG:
        assert case["rows"].shape[1] > 64 * 16   # more chunks than the sums kernel has threads


@pytest.mark.parametrize("name", ["same", "leaves", "many", "zeros"])
def test_special_cases(ctx, name):
    case = TE.extra_cases()[name]
    if name == "many":
        assert len(case["cand"]) == 70001 > 65535 and not R.same_bits(case["want"]["rho"][0], case["want"]["rho"][2])
    if name == "same":
        assert len({tuple(c) for c in case["cand"].tolist()}) == 1 and not R.same_bits(case["want"]["rho"][0], case["want"]["rho"][1])
    if name == "zeros":
        assert case["want"]["any_d0"] and np.all(case["want"]["rho"][3:5] == 0.0)
    check(ctx, case, name)


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 4), (20, 17, "inner3", 2), (61, 15, "balanced8", 2), (64, 33, "balanced8", 1), (4, 17, "caterpillar96", 1)])
def test_own_matrices_give_the_plain_entry_and_the_site_values_the_rates_entry(ctx, key):
    case = E.make_case(*key, own=True)
    nedges, ncols, ncat = len(case["parent"]) - 1, case["rows"].shape[1], case["ncat"]
    new = check(ctx, case, key)
    old = ctx.tree_nni(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["cand"],
                       out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full((len(case["cand"]), ncols), GARBAGE_F)))
    assert R.same_bits(new[3], old[3]) and R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and R.same_bits(new[2], old[2])
    rates = ctx.tree_likelihood_rates(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=False,
                                      out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], rates[0]) and np.array_equal(new[1], rates[1]) and R.same_bits(new[2], rates[2])
    if ncat == 1:
        assert case["w"].tolist() == [1.0]
        plain = ctx.tree_likelihood(case["dim"], case["parent"], case["rows"], case["pi"], case["P"], derivs=False,
                                    out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
        assert R.same_bits(new[0], plain[0]) and np.array_equal(new[1], plain[1]) and np.all(new[2] == 1.0)


def test_calls_of_different_shapes_on_one_context(ctx):
    """Large, small, large again, the four other entries in between: nothing of a call is read by the next (the entries share their
    scratch buffers)."""
    import test_gpu_mlancestral as TA
    import test_gpu_mlgamma as TR
    import test_gpu_mlsearch as TN
    import test_gpu_mltree as TO
    import treelik_anc_ref as A
    import treelik_rates_ref as G
    order = [("edge", (20, 33, "balanced24", 4)), ("nni", (20, 33, "balanced8", 4)), ("edge", (4, 1, "balanced8", 2)), ("old", (20, 300, "balanced8")), ("edge", (64, 33, "balanced8", 4)),
             ("rates", (20, 33, "balanced8", 4)), ("edge", (4, 17, "caterpillar96", 1)), ("anc", (4, 300, "balanced8", 4)), ("edge", (4, 33, "balanced8", 4, "one")),
             ("nni", (4, 17, "caterpillar96", 1)), ("edge", (20, 33, "balanced24", 4))]
    for k, (which, key) in enumerate(order):
        what = ("call %d" % k,) + key
        if which == "edge":
            check(ctx, E.make_case(*key), what)
        elif which == "nni":
            TN.check(ctx, N.make_case(*key), what)
        elif which == "anc":
            TA.check(ctx, A.make_case(*key), what)
        elif which == "rates":
            TR.check(ctx, G.make_case(*key), what)
        else:
            TO.check(ctx, R.make_case(*key), what)


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = E.make_case(*TE.SMALL_VALID)
    parent, rows, pi, w, Pm, Pc = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["w"].copy(), case["P"].copy(), case["Pc"].copy()
    cv, ca, cc = (np.ascontiguousarray(case["cand"][:, k]) for k in range(3))
    outs = garbage(2, 15, 12)
    f = pg.lib.pgm_tree_nni_edge
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double), 12,
            P(cv, C.c_uint32), P(ca, C.c_uint32), P(cc, C.c_uint32), P(Pc, C.c_double), P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double),
            P(outs[3], C.c_double), P(outs[4], C.c_double), P(outs[5], C.c_double)]
    bad, keep = [], []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 4, 6, 7, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21):   # null pointers (Pc, d1 and d2 among them)
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
    assert all(np.all(o == (GARBAGE_I if o.dtype == np.int32 else GARBAGE_F)) for o in outs)
    # the context is as good as before
    assert f(*args) == 0
    want = case["want"]
    assert R.same_bits(outs[0], want["site_l"]) and np.array_equal(outs[1], want["site_k"]) and R.same_bits(outs[2], want["post"]) and R.same_bits(outs[3], want["rho"])
    assert R.same_bits(outs[4], want["d1"]) and R.same_bits(outs[5], want["d2"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0
    for wrong in (dict(pi=pi[:3]), dict(P=Pm[:-1]), dict(w=w.reshape(1, 2)), dict(cand=case["cand"][:, :2]), dict(Pc=Pc[:-1])):   # the binding's own checks
        kw = dict(pi=pi, w=w, P=Pm, cand=case["cand"], Pc=Pc); kw.update(wrong)
        with pytest.raises(ValueError):
            ctx.tree_nni_edge(4, parent, rows, kw["pi"], kw["w"], kw["P"], kw["cand"], kw["Pc"])
    with pytest.raises(ValueError):
        ctx.tree_nni_edge(4, parent, rows, pi, w, Pm, case["cand"], Pc, out=outs[:5] + (np.zeros(11),))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


fams = TSUP.fams
starts = TE.starts


def run_both(exe, fa, d, tag, opts, search=None, start=None, reps=50, env=None):
    """A run with --ml_support (and --ml_search N with its log): the files and the stats."""
    log = os.path.join(str(d), tag + ".log")
    extra = (["--ml_search", str(search), "--ml_search_log", log] if search is not None else []) + (["--ml_start", start] if start else [])
    r = TSUP.run_sup(exe, fa, d, tag, list(opts) + extra, reps=reps, env=env)
    r.log_text = open(log).read() if os.path.exists(log) else None
    return r


FILES = lambda r: (r.tree, r.sites, r.log_text, r.support, r.table, r.stdout)


@pytest.mark.parametrize("gamma", [[], ["--ml_gamma", "4"]])
@pytest.mark.parametrize("flows", ["search", "support", "both"])
def test_driver_equals_the_oracle_driver(exe, oracle_build, starts, tmp_path, gamma, flows):
    """The 8-taxon fixtures with the device switch, from both splits of a clade of four wrong: the tree, the sites file, the log, the
    support tree, the table and ml_lnl of the product driver are the oracle driver's (the host loops), byte for byte."""
    fams = starts
    opts = TS.DNA(fams) + gamma + ["--ml_nni_opt", "5"]
    env = dict(os.environ, PGM_DEVICE_TREELIK="1")
    oracle = os.path.join(oracle_build, "pgmsa_oracle")
    if flows == "search":
        got = TS.run_s(exe, fams["sim8"], tmp_path, "hip", opts, search=10, start=fams["swapped_pair"], env=env)
        ref = TS.run_s(oracle, fams["sim8"], tmp_path, "ref", opts, search=10, start=fams["swapped_pair"])
        assert (got.tree, got.sites, got.log_text, got.stdout) == (ref.tree, ref.sites, ref.log_text, ref.stdout) and len(got.log) >= 2
    else:
        search = 10 if flows == "both" else None
        got = run_both(exe, fams["sim8"], tmp_path, "hip", opts, search=search, start=fams["swapped_pair" if search else "one"], env=env)
        ref = run_both(oracle, fams["sim8"], tmp_path, "ref", opts, search=search, start=fams["swapped_pair" if search else "one"])
        assert FILES(got) == FILES(ref) and got.support is not None and got.table is not None
        assert got.stats["ml_support_kernel_ms"] > 0
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert got.stats["ml_lnl"] == ref.stats["ml_lnl"] and got.stats["ml_nni_opt_calls"] == ref.stats["ml_nni_opt_calls"] > 0
    assert got.stats["ml_nni_opt_kernel_ms"] > 0 and ref.stats["ml_nni_opt_kernel_ms"] == 0
    if flows != "support":
        assert N.bipartitions(got.tree) == N.bipartitions(TS.TRUE8) and got.stats["ml_nni_calls"] == ref.stats["ml_nni_calls"]


def test_default_route_by_size(exe, oracle_build, starts, tmp_path_factory, tmp_path):
    """8 taxa take the host loop by default and 24 the device; PGM_HOST_TREELIK keeps the host loop at 24: the same files either way."""
    fams = starts
    d = tmp_path_factory.mktemp("mlo_route")
    aa24 = [f for f in bu.aa_families(d) if f.endswith("_n24.fa")][0]
    opts = ["--ml_nni_opt", "2"]
    got = run_both(exe, aa24, tmp_path, "hip", opts, search=2, reps=20)
    ref = run_both(os.path.join(oracle_build, "pgmsa_oracle"), aa24, tmp_path, "ref", opts, search=2, reps=20)
    host = run_both(exe, aa24, tmp_path, "host", opts, search=2, reps=20, env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert FILES(got) == FILES(ref) == FILES(host)
    assert got.stats["ml_nni_opt_kernel_ms"] > 0 and host.stats["ml_nni_opt_kernel_ms"] == 0 and got.stats["ml_nni_opt_calls"] == host.stats["ml_nni_opt_calls"] >= 6
    small = run_both(exe, fams["sim8"], tmp_path, "small", TS.DNA(fams) + opts, search=10, start=fams["one"], reps=20)
    assert small.stats["ml_nni_opt_kernel_ms"] == 0 and small.stats["ml_kernel_ms"] == 0 and small.stats["ml_nni_opt_calls"] >= 6
