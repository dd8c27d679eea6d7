"""pgm_resampled_sums on the MI355X against tests/resample_ref.py: equality bit for bit, out preset to garbage; then `pgmsa --ml_tree
--ml_support --stats` against pgmsa_oracle byte for byte.

The cases (tests/resample_ref.py and tests/test_cpu_mlsupport.py hold the lists; the stand-alone host program runs the same ones).  A
wavefront of the sums' kernel owns T = 64 rows (one a lane) and 4 replicates, a workgroup 16 replicates, and the transpose works in
32 x 32 tiles: rows of {1, 2, 63, 64, 65, 257} sit on both sides of a q-tile's edge and reach several tiles, columns of {1, 2, 17, 257,
2891} on both sides of the transpose's tile and of the unrolled loop's step, replicates of {1, 2, 63, 64, 65, 1000} on both sides of a
wavefront's four and a workgroup's sixteen; 70001 rows x 3 columns x 2 replicates are 1094 q-tiles; 1000 replicates of 65 rows are 8 x
63 = 504 items and 257 rows of 65 replicates 40, so the 2048-workgroup grid strides only in the case made for it.  Values: all one
column, the identity, rows that hold -infinity, and magnitudes from 1e-300 to 1e300 of both signs, where any other order of the
additions would show.  The expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import resample_ref as RS
import test_cpu_mlsupport as TS
import test_cpu_mlsearch as TN
import treelik_nni_ref as N
import treelik_ref as R

pytestmark = pytest.mark.gpu

GARBAGE = -7.25e77


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def check(ctx, key):
    x, cols, want = RS.make_case(*key)
    assert not np.any(np.isnan(want)) and not np.any(want == np.inf)
    out = ctx.resampled_sums(x, cols, out=np.full(want.shape, GARBAGE))
    assert R.same_bits(out, want), key
    return out


@pytest.mark.parametrize("key", [c for c in TS.SUM_CASES if c[0] != 70001])
def test_sums_equal_the_statement(ctx, key):
    check(ctx, key)


def test_more_items_than_the_grid_holds(ctx):
    """70001 rows: 1094 q-tiles.  With 40 replicates they make 1096 x 3 = 3288 items for 2048 workgroups, so 1240 of them take a second
    item; with 2 replicates (the issue's shape) every q-tile has one item."""
    check(ctx, (70001, 3, 2, "random"))
    x, cols, _ = RS.make_case(70001, 3, 2)
    cols40 = RS.make_case(1, 3, 40)[1]
    want = RS.sums(x, cols40)
    assert (70001 + 63) // 64 == 1094 and (1094 + 7) // 8 * 8 * 3 > 2048
    out = ctx.resampled_sums(x, cols40, out=np.full(want.shape, GARBAGE))
    assert R.same_bits(out, want)


def test_values_of_every_kind(ctx):
    for kind in RS.KINDS[1:]:
        x, cols, want = RS.make_case(65, 17, 5, kind)
        out = check(ctx, (65, 17, 5, kind))
        if kind == "minus infinity":
            assert np.all(out[32] == -np.inf) and np.any(np.isfinite(out))
        if kind == "one column":
            assert np.all(cols == 16)
        if kind == "identity":
            assert all(R.same_bits(out[:, 0], out[:, r]) for r in range(5))
        if kind == "mixed magnitude":   # the same terms added in the reverse order give other bits on these values
            assert not R.same_bits(out, RS.sums(x, cols[:, ::-1]))


def test_calls_of_different_shapes_on_one_context(ctx):
    """Large, small, large again, a tree_nni call in between: nothing of a call is read by the next."""
    import test_gpu_mlsearch as TG
    check(ctx, (257, 257, 65, "random"))
    check(ctx, (1, 1, 1, "random"))
    TG.check(ctx, N.make_case(20, 33, "balanced8", 4), "between")
    check(ctx, (65, 2891, 3, "random"))
    check(ctx, (3, 17, 1000, "random"))
    TG.check(ctx, N.make_case(4, 17, "balanced8", 1), "between")
    check(ctx, (257, 257, 65, "mixed magnitude"))


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    x, cols, want = RS.make_case(3, 5, 2)
    x, cols = np.array(x), np.array(cols)
    out = np.full((3, 2), GARBAGE)
    f = pg.lib.pgm_resampled_sums
    args = [ctx.handle, 3, 5, P(x, C.c_double), 2, P(cols, C.c_uint32), P(out, C.c_double)]
    bad, keep = [], []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 3, 5, 6):                                    # null pointers
        call({k: None})
    for k in (1, 2, 4):                                       # nrow, ncols, nrep == 0
        call({k: 0})
    call({1: 65536, 2: 1, 4: 65536})                          # nrow * nrep beyond 32 bits
    call({1: 1, 2: 65536, 4: 65536})                          # nrep * ncols beyond 32 bits
    call({1: 0xFFFFFFFF, 4: 2})
    for _, c in RS.bad_calls():                               # a cols entry >= ncols
        keep.append(c)
        call({5: P(c, C.c_uint32)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(out == GARBAGE)
    # the context is as good as before
    assert f(*args) == 0
    assert R.same_bits(out, want)
    assert pg.lib.pgm_resample_last_kernel_ms(ctx.handle) > 0
    for wrong in (dict(x=x[0]), dict(cols=cols[:, :4]), dict(cols=cols[0])):   # the binding's own checks
        kw = dict(x=x, cols=cols); kw.update(wrong)
        with pytest.raises(ValueError):
            ctx.resampled_sums(kw["x"], kw["cols"])
    with pytest.raises(ValueError):
        ctx.resampled_sums(x, cols, out=np.zeros((2, 3)))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


fams = TS.fams


@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"], ["--ml_search", "10"], ["--ml_gamma", "4", "--ml_search", "10"]])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, opts):
    """The 8-taxon fixtures with the device switch, from one interchange away: the support tree, the table, the --ml_tree file and
    ml_lnl of the product driver are the oracle driver's (the host loops), byte for byte."""
    opts = TS.DNA(fams) + ["--ml_start", fams["one"]] + opts
    env = dict(os.environ, PGM_DEVICE_TREELIK="1")
    got = TS.run_sup(exe, fams["sim8"], tmp_path, "hip", opts, reps=200, env=env)
    ref = TS.run_sup(os.path.join(oracle_build, "pgmsa_oracle"), fams["sim8"], tmp_path, "ref", opts, reps=200)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert got.support is not None and got.table is not None and len(got.nodes) == 4
    assert (got.support, got.table, got.tree, got.sites, got.stdout) == (ref.support, ref.table, ref.tree, ref.sites, ref.stdout)
    assert got.stats["ml_lnl"] == ref.stats["ml_lnl"]
    for k in ("ml_support_nodes", "ml_support_calls", "ml_rounds", "ml_evaluations"):
        assert got.stats[k] == ref.stats[k], k
    assert got.stats["ml_support_kernel_ms"] > 0 and ref.stats["ml_support_kernel_ms"] == 0
    if "--ml_search" in opts:
        assert got.stats["ml_nni_calls"] == ref.stats["ml_nni_calls"] and N.bipartitions(got.tree) == N.bipartitions(TN.TRUE8)
    assert "PGM_DEVICE_TREELIK" in got.stats["switches"]


def test_zero_length_branch_on_the_device(exe, oracle_build, fams, tmp_path):
    opts = TS.DNA(fams) + ["--ml_start", fams["zero"]]
    got = TS.run_sup(exe, fams["zero8"], tmp_path, "hip", opts, env=dict(os.environ, PGM_DEVICE_TREELIK="1"))
    ref = TS.run_sup(os.path.join(oracle_build, "pgmsa_oracle"), fams["zero8"], tmp_path, "ref", opts)
    assert (got.support, got.table, got.tree) == (ref.support, ref.table, ref.tree) and got.stats["ml_support_kernel_ms"] > 0


def test_default_route_by_size(exe, oracle_build, fams, tmp_path_factory, tmp_path):
    """8 taxa take the host loops by default and 24 the device; PGM_HOST_TREELIK keeps the host loops at 24: the same files either way."""
    d = tmp_path_factory.mktemp("mlsup_route")
    aa24 = [f for f in bu.aa_families(d) if f.endswith("_n24.fa")][0]
    got = TS.run_sup(exe, aa24, tmp_path, "hip", reps=100)
    ref = TS.run_sup(os.path.join(oracle_build, "pgmsa_oracle"), aa24, tmp_path, "ref", reps=100)
    host = TS.run_sup(exe, aa24, tmp_path, "host", reps=100, env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (got.support, got.table, got.tree) == (ref.support, ref.table, ref.tree) == (host.support, host.table, host.tree)
    assert got.stats["ml_support_kernel_ms"] > 0 and host.stats["ml_support_kernel_ms"] == 0 and got.stats["ml_support_calls"] == 1
    assert len(got.nodes) >= 20
    small = TS.run_sup(exe, fams["sim8"], tmp_path, "small", TS.DNA(fams), reps=100)
    assert small.stats["ml_support_kernel_ms"] == 0 and small.stats["ml_kernel_ms"] == 0 and small.stats["ml_support_calls"] == 1
