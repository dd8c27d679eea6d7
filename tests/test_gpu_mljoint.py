"""pgm_tree_ancestral_joint and pgm_tree_ancestral_sample on the MI355X against tests/treelik_joint_ref.py: site_l, site_k, post and
joint_l bit for bit, cat, joint_state, joint_k, samp_cat and samp_state as integers, every output preset to garbage; then `pgmsa
--ml_tree --ml_ancestral_joint --ml_ancestral_samples` against pgmsa_oracle byte for byte.

The joint cases: every dim of {4, 20, 61, 64} with ncat of {1, 4} and ncols of {1, 17, 33} on the balanced tree of 8 leaves (one and
several workgroups of the max pass, a last workgroup with idle lanes: 61 states leave three lanes idle, 17 columns of 4 states fill a
sixteenth of the second workgroup); the trees of 2 leaves (the root alone: no back-pointer), 3 and 24 leaves and the trifurcating root;
300 columns of 4 states (five workgroups of the thread-per-site traceback); the caterpillar of 96 leaves, where joint_k > 0 and differs
from site_k; a workgroup of the max pass whose sites read different categories' matrices; a tie; impossible columns.  The sampler: nsamp
around one wavefront of samples, two seeds, first_sample 0 and 7, dims {4, 20, 64}, ncat {1, 4}, and the -1 propagation.  The
expectations are computed once per process; tests/test_cpu_mljoint.py puts the same cases to the host loops."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mljoint as TJ
import treelik_joint_ref as J
import treelik_ref as R

pytestmark = pytest.mark.gpu

GARBAGE_F, GARBAGE_I, GARBAGE_B, GARBAGE_U = -7.25e77, -77777, -99, 201


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncat, ncols, ninner):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full(ncols, GARBAGE_U, np.uint8),
            np.full((ninner, ncols), GARBAGE_B, np.int8), np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32))


def garbage_samples(ncat, ncols, ninner, nsamp):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((ncat, ncols), GARBAGE_F), np.full((ncols, nsamp), GARBAGE_U, np.uint8),
            np.full((ninner, ncols, nsamp), GARBAGE_B, np.int8))


def site_values(out, want, what):
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    assert R.same_bits(out[2], want["post"]), what


def check(ctx, case, what):
    ninner, ncols = len(case["parent"]) - case["nleaves"], case["rows"].shape[1]
    out = ctx.tree_ancestral_joint(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], out=garbage(case["ncat"], ncols, ninner))
    want = case["want"]
    site_values(out, want, what)
    assert np.array_equal(out[3], want["cat"]), what
    assert np.array_equal(out[4], want["joint_state"]), what
    assert R.same_bits(out[5], want["joint_l"]), what
    assert np.array_equal(out[6], want["joint_k"]), what
    return out


def check_samples(ctx, case, key, nsamp, seed, first, what):
    """The samples first .. first + nsamp - 1 are those columns of the statement's samples 0 .. 136 (its own independence of the cut:
    tests/test_cpu_mljoint.py)."""
    ninner, ncols = len(case["parent"]) - case["nleaves"], case["rows"].shape[1]
    want = J.samples_of(case, 137, seed, 0, key=key)
    out = ctx.tree_ancestral_sample(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], nsamp, seed, first_sample=first,
                                    out=garbage_samples(case["ncat"], ncols, ninner, nsamp))
    site_values(out, want, what)
    assert np.array_equal(out[3], want["samp_cat"][:, first:first + nsamp]), what
    assert np.array_equal(out[4], want["samp_state"][:, :, first:first + nsamp]), what
    return out


# ---- joint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", TJ.GRID)
def test_balanced_tree_of_8(ctx, key):
    check(ctx, J.make_case(*key), key)


@pytest.mark.parametrize("key", TJ.OTHER_TREES)
def test_other_trees(ctx, key):
    check(ctx, J.make_case(*key), key)


def test_more_than_one_workgroup_of_the_traceback(ctx):
    check(ctx, J.make_case(*TJ.MANY_COLUMNS), "300 columns")


def test_caterpillar_rescales_the_maxima(ctx):
    out = check(ctx, J.make_mixed_scaling_case(*TJ.MIXED_SCALING), "mixed scaling")
    assert np.any(out[6] > 0) and np.any(out[6] != out[1])


def test_categories_vary_within_a_workgroup(ctx):
    out = check(ctx, J.make_case(*TJ.VARYING_CATEGORY), "varying category")
    assert len(set(out[3][:16].tolist())) > 1   # (4 states: the first workgroup of the max pass owns the columns 0 .. 15)


def test_ties_and_impossible_columns(ctx):
    out = check(ctx, J.with_want(TJ.tie_case()), "tie")
    assert np.all(out[4] == 1)
    out = check(ctx, J.with_want(TJ.degenerate_case(1)), "degenerate, one category")
    assert out[5].tolist() == [0.0, 0.0, 0.2, 0.4] and out[4].T.tolist() == [[-1, -1], [-1, -1], [1, 1], [3, 3]]
    out = check(ctx, J.with_want(TJ.degenerate_case(2)), "degenerate, two categories")
    assert out[3][:2].tolist() == [1, 1] and np.all(out[4] >= 0)


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 4), (61, 17, "balanced8", 1), (20, 33, "balanced24", 4)])
def test_site_values_equal_the_rates_entry(ctx, key):
    case = J.make_case(*key)
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    new = check(ctx, case, key)
    old = ctx.tree_likelihood_rates(case["dim"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=False,
                                    out=(np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full((case["ncat"], ncols), GARBAGE_F), np.full(nedges, GARBAGE_F),
                                         np.full(nedges, GARBAGE_F)))
    assert R.same_bits(new[0], old[0]) and np.array_equal(new[1], old[1]) and R.same_bits(new[2], old[2])
    drawn = check_samples(ctx, case, key, 5, 9, 0, key)
    assert R.same_bits(drawn[0], old[0]) and np.array_equal(drawn[1], old[1]) and R.same_bits(drawn[2], old[2])


# ---- sample -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", TJ.SAMPLE_KEYS)
def test_samples(ctx, key):
    case = J.make_case(*key)
    for seed in TJ.SAMPLE_SEEDS:
        for nsamp in TJ.SAMPLE_COUNTS:
            for first in TJ.SAMPLE_FIRSTS:
                check_samples(ctx, case, key, nsamp, seed, first, key + (nsamp, seed, first))
    a = J.samples_of(case, 137, TJ.SAMPLE_SEEDS[0], 0, key=key)["samp_state"]
    assert not np.array_equal(a, J.samples_of(case, 137, TJ.SAMPLE_SEEDS[1], 0, key=key)["samp_state"]) and np.all(a >= 0)


@pytest.mark.parametrize("ncat", [1, 2])
def test_samples_of_impossible_columns(ctx, ncat):
    case = TJ.degenerate_case(ncat)
    out = check_samples(ctx, case, "degenerate%d" % ncat, 70, 3, 0, "degenerate")
    if ncat == 1:
        assert np.all(out[3][:2] == 255) and np.all(out[4][:, :2] == -1) and np.all(out[4][:, 2] == 1) and np.all(out[4][:, 3] == 3)
    else:
        assert np.all(out[3][:2] == 1) and np.all(out[4] >= 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _bad_calls(f, args, null_at, parent_at, rows_at, w_at, ncat_at, parent, rows, w, extra):
    bad, keep = [], []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in null_at:
        call({k: None})
    for k, v in ((ncat_at, 0), (ncat_at, 17), (ncat_at, 0xFFFFFFFF)):       # ncat outside 1 .. 16
        call({k: v})
    for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):      # a weight that is not finite and > 0
        ww = w.copy(); ww[1] = v; keep.append(ww)
        call({w_at: P(ww, C.c_double)})
    for k, v in ((1, 0), (1, 65), (2, 1), (2, 0), (5, 0), (3, 8), (3, 7)):   # what the likelihood entries refuse
        call({k: v})
    for changes in ({8: 8}, {8: 3}, {9: 15}, {0: 3}, {0: 9}, {13: 0xFFFFFFFF}):
        p = parent.copy()
        for k, v in changes.items():
            p[k] = v
        keep.append(p)
        call({parent_at: P(p, C.c_uint32)})
    for v in (4, -3, 127, -128):
        r = rows.copy(); r[7, 14] = v; keep.append(r)
        call({rows_at: P(r, C.c_int8)})
    for changes in extra:
        call(changes)
    return bad


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = J.make_case(*TJ.SMALL_VALID)
    parent, rows, pi, w, Pm = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["w"].copy(), case["P"].copy()
    outs = garbage(2, 15, 7)
    f = pg.lib.pgm_tree_ancestral_joint
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double),
            P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_uint8), P(outs[4], C.c_int8), P(outs[5], C.c_double), P(outs[6], C.c_int32)]
    bad = _bad_calls(f, args, (0, 4, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17), 4, 6, 9, 8, parent, rows, w, [])
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(outs[0] == GARBAGE_F) and np.all(outs[1] == GARBAGE_I) and np.all(outs[2] == GARBAGE_F) and np.all(outs[3] == GARBAGE_U)
    assert np.all(outs[4] == GARBAGE_B) and np.all(outs[5] == GARBAGE_F) and np.all(outs[6] == GARBAGE_I)
    assert f(*args) == 0   # the context is as good as before
    assert R.same_bits(outs[5], case["want"]["joint_l"]) and np.array_equal(outs[4], case["want"]["joint_state"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0

    souts = garbage_samples(2, 15, 7, 3)
    g = pg.lib.pgm_tree_ancestral_sample
    sargs = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), 2, P(w, C.c_double), P(Pm, C.c_double), 3, 0, 1,
             P(souts[0], C.c_double), P(souts[1], C.c_int32), P(souts[2], C.c_double), P(souts[3], C.c_uint8), P(souts[4], C.c_int8)]
    bad = _bad_calls(g, sargs, (0, 4, 6, 7, 9, 10, 14, 15, 16, 17, 18), 4, 6, 9, 8, parent, rows, w, [{11: 0}])   # ... and no sample
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(souts[0] == GARBAGE_F) and np.all(souts[1] == GARBAGE_I) and np.all(souts[2] == GARBAGE_F) and np.all(souts[3] == GARBAGE_U) and np.all(souts[4] == GARBAGE_B)
    assert g(*sargs) == 0
    want = J.samples_of(case, 137, 1, 0, key=TJ.SMALL_VALID)
    assert np.array_equal(souts[4], want["samp_state"][:, :, :3]) and np.array_equal(souts[3], want["samp_cat"][:, :3])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0
    for wrong in (dict(pi=pi[:3]), dict(P=Pm[:-1]), dict(w=w.reshape(1, 2))):   # the binding's own checks
        kw = dict(pi=pi, w=w, P=Pm); kw.update(wrong)
        with pytest.raises(ValueError):
            ctx.tree_ancestral_joint(4, parent, rows, kw["pi"], kw["w"], kw["P"])
        with pytest.raises(ValueError):
            ctx.tree_ancestral_sample(4, parent, rows, kw["pi"], kw["w"], kw["P"], 3, 1)
    with pytest.raises(ValueError):
        ctx.tree_ancestral_sample(4, parent, rows, pi, w, Pm, 0, 1)
    with pytest.raises(ValueError):
        ctx.tree_ancestral_joint(4, parent, rows, pi, w, Pm, out=outs[:6])


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fam24(tmp_path_factory):
    import gen
    d = tmp_path_factory.mktemp("mlj_fam")
    fa = str(d / "n24.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta(gen.gen(24, 300, 5)))
    return fa


@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"], ["--ml_search", "3"]])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fam24, tmp_path, opts):
    """gen.py 24 300 5: 24 taxa take the device route by default.  The three files, the other outputs and the likelihoods of the product
    driver are the oracle driver's (the host loops), byte for byte; with PGM_HOST_TREELIK the product driver runs the host loops too."""
    opts = ["-i", "0"] + opts
    got = TJ.run_j(exe, fam24, tmp_path, "hip", opts, samples=5)
    ref = TJ.run_j(os.path.join(oracle_build, "pgmsa_oracle"), fam24, tmp_path, "ref", opts, samples=5)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert (got.joint, got.jsites, got.samples) == (ref.joint, ref.jsites, ref.samples)
    assert (got.tree, got.sites, got.rates, got.stdout) == (ref.tree, ref.sites, ref.rates, ref.stdout)
    assert len(got.joint) > 0 and len(got.jsites) > 0 and got.samples.count(">") == 5 * 23
    assert got.stats["ml_kernel_ms"] > 0 and ref.stats["ml_kernel_ms"] == 0 and got.stats["ml_ancestral_joint_s"] > 0 and got.stats["ml_ancestral_samples_s"] > 0
    without = TJ.run_j(exe, fam24, tmp_path, "without", opts, joint=False, samples=0)
    assert "ml_ancestral_joint_s" not in without.stats and "ml_ancestral_samples_s" not in without.stats and without.stats["ml_kernel_ms"] < got.stats["ml_kernel_ms"]
    assert (without.tree, without.sites, without.stdout) == (got.tree, got.sites, got.stdout)
    host = TJ.run_j(exe, fam24, tmp_path, "host", opts, samples=5, env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (host.joint, host.jsites, host.samples) == (got.joint, got.jsites, got.samples) and host.stats["ml_kernel_ms"] == 0
