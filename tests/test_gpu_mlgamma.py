"""pgm_tree_likelihood_rates on the MI355X against tests/treelik_rates_ref.py: equality of site_l, site_k, post, d1 and d2 bit for bit,
every output preset to garbage; then `pgmsa --ml_tree --ml_gamma --stats` against pgmsa_oracle byte for byte.

The cases: every dim of {4, 20, 61, 64} with ncat of {1, 2, 4, 16} and ncols of {1, 17, 33} (around the chunk of 16; more than one
workgroup of the walk from dim 4 x 17 on, one workgroup of the combine kernel) on the balanced tree of 8 leaves; ncat = 4 and 33
columns on the trees of 2, 3 and 24 leaves and the trifurcating root; 300 columns (five workgroups of the combine kernel); a
caterpillar of 96 leaves whose two categories rescale a different number of times (the shift by 2^-256, once and to an exact 0.0).
Category 0 of every case is treelik_ref's case, so the inputs hold its column of gaps, row of gaps and -2 entries; the
expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mlgamma as TG
import test_cpu_mltree as TM
import treelik_rates_ref as G
import treelik_ref as R

pytestmark = pytest.mark.gpu

DIMS = (4, 20, 61, 64)
GARBAGE_F, GARBAGE_I = -7.25e77, -77777


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncat, ncols, nedges):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F))


def check(ctx, case, what):
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    out = ctx.tree_likelihood_rates(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=case["derivs"],
                                    out=garbage(case["ncat"], ncols, nedges))
    want = case["want"]
    assert not np.any(np.isnan(want["site_l"])) and not np.any(np.isnan(want["post"]))
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    assert R.same_bits(out[2], want["post"]), what
    if case["derivs"]:
        assert not np.any(np.isnan(want["d1"])) and not np.any(np.isnan(want["d2"]))
        assert R.same_bits(out[3], want["d1"]) and R.same_bits(out[4], want["d2"]), what
    else:
        assert np.all(out[3] == GARBAGE_F) and np.all(out[4] == GARBAGE_F), what   # untouched
    return out


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("ncat", [1, 2, 4, 16])
@pytest.mark.parametrize("ncols", [1, 17, 33])
def test_balanced_tree_of_8(ctx, dim, ncat, ncols):
    check(ctx, G.make_case(dim, ncols, "balanced8", ncat), (dim, ncat, ncols))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("tree", ["two", "three", "balanced24", "trifurcating"])
def test_other_trees(ctx, dim, tree):
    check(ctx, G.make_case(dim, 33, tree, 4), (dim, tree))


def test_more_than_one_workgroup_of_the_combine_kernel(ctx):
    check(ctx, G.make_case(4, 300, "balanced8", 4), "300 columns")


def test_mixed_scaling(ctx):
    """k_0 > k_1 on the columns without gaps: category 0's term is shifted by 2^-256, its posterior is tiny but the statement's."""
    case = G.make_mixed_scaling_case(4)
    out = check(ctx, case, "mixed scaling")
    hit = case["full"] & (case["diff"] >= 1)
    assert hit.any() and np.all(out[2][0][hit] > 0) and np.all(out[2][0][hit] < 1e-60)
    assert np.array_equal(out[1], case["want"]["cat_k"].min(axis=0))


@pytest.mark.parametrize("dim", [4, 20])
def test_mixed_scaling_to_an_exact_zero(ctx, dim):
    case = G.make_mixed_scaling_case(dim, 1e-6, 5)
    out = check(ctx, case, "mixed scaling, five shifts and more")
    hit = case["full"] & (case["diff"] >= 5)
    assert hit.any() and np.all(out[2][0][hit] == 0.0) and np.all(out[2][1][hit] == 1.0)


@pytest.mark.parametrize("key", [(4, 33, "balanced8"), (20, 17, "balanced8"), (61, 33, "trifurcating"), (64, 17, "caterpillar96")])
def test_one_category_equals_the_old_entry(ctx, key):
    case = G.make_case(*key, 1)
    assert case["w"].tolist() == [1.0]
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood(case["dim"], case["parent"], case["rows"], case["pi"], case["P"], derivs=True,
                              out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and R.same_bits(new[3], old[2]) and R.same_bits(new[4], old[3])
    assert np.all(new[2] == 1.0)


def test_unequal_weights(ctx):
    case = G.make_case(4, 33, "balanced8", 4, True, "unequal")
    assert case["w"].tolist() == [0.1, 0.2, 0.3, 0.4]
    out = check(ctx, case, "unequal weights")
    assert not R.same_bits(out[0], G.make_case(4, 33, "balanced8", 4)["want"]["site_l"])


@pytest.mark.parametrize("dim,ncols,tree,ncat", [(20, 33, "balanced8", 4), (61, 17, "balanced8", 2), (4, 17, "caterpillar96", 2), (64, 33, "trifurcating", 4)])
def test_without_derivatives(ctx, dim, ncols, tree, ncat):
    case = G.make_case(dim, ncols, tree, ncat, False)
    check(ctx, case, (dim, ncols, tree, ncat, "no derivs"))
    with_d = G.make_case(dim, ncols, tree, ncat)
    assert R.same_bits(case["want"]["site_l"], with_d["want"]["site_l"]) and R.same_bits(case["want"]["post"], with_d["want"]["post"])   # (the same up pass)


def test_calls_of_different_shapes_on_one_context(ctx):
    """Large, small, large again, other numbers of categories, the entry without categories in between: nothing of a call is read by
    the next (the two entries share their scratch buffers)."""
    order = [("new", (20, 33, "balanced8", 16)), ("old", (20, 300, "balanced8")), ("new", (4, 1, "balanced8", 2)), ("new", (64, 33, "balanced24", 4)),
             ("old", (4, 17, "caterpillar96")), ("new", (20, 33, "balanced8", 4, False)), ("new", (4, 300, "balanced8", 4)), ("old", (64, 33, "balanced24")),
             ("new", (4, 17, "balanced8", 1)), ("new", (20, 33, "balanced8", 16))]
    import test_gpu_mltree as TO
    for k, (which, key) in enumerate(order):
        if which == "new":
            check(ctx, G.make_case(*key), ("call %d" % k,) + key)
        else:
            TO.check(ctx, R.make_case(*key), ("call %d" % k,) + key)


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = G.make_case(4, 15, "balanced8", 2)
    parent, rows, pi, w, Pm = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["w"].copy(), case["P"].copy()
    outs = garbage(2, 15, 14)
    f = pg.lib.pgm_tree_likelihood_rates
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double), 1,
            P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_double), P(outs[4], C.c_double)]
    bad, keep = [], []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 4, 6, 7, 9, 10, 12, 13, 14, 15, 16):                    # null pointers (w and post among them; d1, d2: the call asks for derivatives)
        call({k: None})
    for k, v in ((8, 0), (8, 17), (8, 0xFFFFFFFF)):                       # ncat outside 1 .. 16
        call({k: v})
    for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):      # a weight that is not finite and > 0
        ww = w.copy(); ww[1] = v; keep.append(ww)
        call({9: P(ww, C.c_double)})
    for k, v in ((1, 0), (1, 65), (2, 1), (2, 0), (5, 0), (3, 8), (3, 7)):   # what the entry without categories refuses
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
    assert np.all(outs[0] == GARBAGE_F) and np.all(outs[1] == GARBAGE_I) and np.all(outs[2] == GARBAGE_F) and np.all(outs[3] == GARBAGE_F) and np.all(outs[4] == GARBAGE_F)
    # d1 and d2 may be null without derivatives, and the context is as good as before
    a = list(args); a[11] = 0; a[15] = None; a[16] = None
    a[10] = P(G.make_case(4, 15, "balanced8", 2, False)["P"], C.c_double)
    assert f(*a) == 0
    assert R.same_bits(outs[0], case["want"]["site_l"]) and R.same_bits(outs[2], case["want"]["post"]) and np.all(outs[3] == GARBAGE_F)
    assert f(*args) == 0
    assert R.same_bits(outs[3], case["want"]["d1"]) and R.same_bits(outs[4], case["want"]["d2"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlg_fams")
    aa = bu.aa_families(d)
    return dict(aa=[f for f in aa if f.endswith("_n24.fa")][0], aa5=[f for f in aa if f.endswith("_n5.fa")][0], dna=bu.dna_families(d), codon=bu.codon_families(d),
                hky=bu.hky_model(d))


def _both(exe, oracle_build, fa, tmp_path, opts, tag):
    """The product driver on the device path and the oracle driver (the host loop): the three files, stdout and the stats."""
    got = TG.run_g(exe, fa, tmp_path, "hip" + tag, opts, env=dict(os.environ, PGM_DEVICE_TREELIK="1"))
    ref = TG.run_g(os.path.join(oracle_build, "pgmsa_oracle"), fa, tmp_path, "ref" + tag, opts)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert (got.tree, got.sites, got.rates, got.stdout) == (ref.tree, ref.sites, ref.rates, ref.stdout)
    assert len(got.tree) > 0 and len(got.sites) > 0 and len(got.rates) > 0
    for k in ("ml_lnl", "ml_lnl_start", "ml_alpha", "ml_categories", "ml_rounds", "ml_evaluations"):
        assert got.stats[k] == ref.stats[k], k
    assert got.stats["ml_kernel_ms"] > 0 and ref.stats["ml_kernel_ms"] == 0 and "PGM_DEVICE_TREELIK" in got.stats["switches"]
    return got, ref


def test_driver_equals_the_oracle_driver_aa(exe, oracle_build, fams, tmp_path):
    got, _ = _both(exe, oracle_build, fams["aa"], tmp_path, ["-i", "0", "--ml_gamma", "4"], "aa")
    TG.check_files(got, "aa", R.shipped("wag.qmat"), 4)
    host = TG.run_g(exe, fams["aa"], tmp_path, "host", ["-i", "0", "--ml_gamma", "4"], env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (host.tree, host.sites, host.rates) == (got.tree, got.sites, got.rates) and host.stats["ml_kernel_ms"] == 0


def test_driver_equals_the_oracle_driver_fixed_alpha(exe, oracle_build, fams, tmp_path):
    got, _ = _both(exe, oracle_build, fams["aa"], tmp_path, ["-i", "0", "--ml_gamma", "4", "--ml_alpha", "0.7"], "fixed")
    assert got.stats["ml_alpha"] == 0.7


def test_driver_equals_the_oracle_driver_dna(exe, oracle_build, fams, tmp_path):
    fa = [f for f in fams["dna"] if len(R.read_fasta(f)) >= 3][0]
    _both(exe, oracle_build, fa, tmp_path, ["--dna", "--custom_model", fams["hky"], "--ml_gamma", "4"], "dna")


def test_driver_equals_the_oracle_driver_codon(exe, oracle_build, fams, tmp_path):
    _both(exe, oracle_build, fams["codon"][1], tmp_path, ["--codon", "--ml_rounds", "3", "--ml_gamma", "2"], "codon")


def test_default_route_by_size(exe, fams, tmp_path):
    """Without a switch the host loop runs below kTreelikDeviceMin = 24 taxa and the device from there on; the same files either way."""
    opts = ["-i", "0", "--ml_gamma", "4", "--ml_alpha", "0.5"]
    small = TG.run_g(exe, fams["aa5"], tmp_path, "small", opts)
    assert small.stats["ml_kernel_ms"] == 0 and small.stats["switches"] == ""
    forced = TG.run_g(exe, fams["aa5"], tmp_path, "forced", opts, env=dict(os.environ, PGM_DEVICE_TREELIK="1"))
    assert forced.stats["ml_kernel_ms"] > 0 and (forced.tree, forced.sites, forced.rates) == (small.tree, small.sites, small.rates)
    large = TG.run_g(exe, fams["aa"], tmp_path, "large", opts)
    assert large.stats["ml_kernel_ms"] > 0 and large.stats["switches"] == ""
