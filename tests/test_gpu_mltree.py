"""pgm_tree_likelihood on the MI355X against tests/treelik_ref.py: equality of site_l, site_k, d1 and d2 bit for bit, every output
preset to garbage; then `pgmsa --ml_tree --ml_sites --stats` against pgmsa_oracle byte for byte.

The cases cover every dim of {4, 20, 61, 64} with every ncols of {1, 15, 16, 17, 33, 300} (around the chunk of 16, more than one
workgroup) on the balanced tree of 8 leaves, every dim on the trees of 2 and 3 leaves, the balanced tree of 24, a trifurcating root
(33 sites each), and every dim on a caterpillar of 96 leaves whose matrices' entries lie in [0.03, 0.07] (17 sites): 0.07^67 < 2^-256,
so every column without missing data must rescale there.  The cases hold a column of gaps, a row of gaps and -2 entries
(treelik_ref.make_case); their expectations are computed once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mltree as TM
import treelik_ref as R

pytestmark = pytest.mark.gpu

DIMS = (4, 20, 61, 64)
NCOLS = (1, 15, 16, 17, 33, 300)
CASES = [(d, n, "balanced8") for d in DIMS for n in NCOLS] + [(d, 33, t) for d in DIMS for t in ("two", "three", "balanced24", "trifurcating")] + \
    [(d, 17, "caterpillar96") for d in DIMS]
GARBAGE_F, GARBAGE_I = -7.25e77, -77777


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def garbage(ncols, nedges):
    return (np.full(ncols, GARBAGE_F), np.full(ncols, GARBAGE_I, np.int32), np.full(nedges, GARBAGE_F), np.full(nedges, GARBAGE_F))


def check(ctx, case, what):
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    out = ctx.tree_likelihood(case["dim"], case["parent"], case["rows"], case["pi"], case["P"], derivs=case["derivs"], out=garbage(ncols, nedges))
    want = case["want"]
    assert R.same_bits(out[0], want["site_l"]), what
    assert np.array_equal(out[1], want["site_k"]), what
    if case["derivs"]:
        assert not np.any(np.isnan(want["d1"])) and not np.any(np.isnan(want["d2"]))
        assert R.same_bits(out[2], want["d1"]) and R.same_bits(out[3], want["d2"]), what
    else:
        assert np.all(out[2] == GARBAGE_F) and np.all(out[3] == GARBAGE_F), what   # untouched
    return out


@pytest.mark.parametrize("dim,ncols,tree", CASES)
def test_equals_the_statement(ctx, dim, ncols, tree):
    case = R.make_case(dim, ncols, tree)
    out = check(ctx, case, (dim, ncols, tree))
    rows = case["rows"]
    if ncols >= 15:
        assert np.all(rows[:, 3] == -1) and np.any(rows == -2)      # the column of gaps, residues without a value
        assert abs(out[0][3] - 1.0) < 1e-9 or tree == "caterpillar96"
    if tree == "caterpillar96":
        full = (rows >= 0).all(axis=0)
        assert full.sum() >= 8 and np.all(out[1][full] > 0)         # the scaling path ran
    else:
        assert np.all(out[1] == 0)


@pytest.mark.parametrize("dim,ncols,tree", [(20, 33, "balanced8"), (61, 17, "balanced8"), (4, 17, "caterpillar96"), (64, 33, "trifurcating")])
def test_without_derivatives(ctx, dim, ncols, tree):
    case = R.make_case(dim, ncols, tree, False)
    check(ctx, case, (dim, ncols, tree, "no derivs"))
    with_d = R.make_case(dim, ncols, tree)
    assert R.same_bits(case["want"]["site_l"], with_d["want"]["site_l"])   # (the same up pass: the cases share rows, pi and P)


def test_calls_of_different_shapes_on_one_context(ctx):
    """Large, small, large again, without derivatives in between: nothing of a call is read by the next (the scratch buffers are
    reused and hold the previous call's partials).  At the end other thread layouts in turn: 3 states (21 sites per wavefront and an
    idle lane) behind 64 (one site), 33 states (one site, 31 idle lanes) behind 2 (32 sites)."""
    order = [(20, 300, "balanced8", True), (4, 1, "balanced8", True), (64, 33, "balanced24", True), (20, 33, "balanced8", False), (4, 33, "two", True),
             (61, 17, "caterpillar96", True), (20, 300, "balanced8", True), (4, 17, "caterpillar96", False), (20, 33, "three", True),
             (64, 17, "balanced8", True), (3, 85, "balanced8", True), (2, 129, "balanced8", True), (33, 5, "balanced8", True)]
    for k, key in enumerate(order):
        check(ctx, R.make_case(*key), ("call %d" % k,) + key)


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    case = R.make_case(4, 15, "balanced8")
    parent, rows, pi, Pm = case["parent"].copy(), case["rows"].copy(), case["pi"].copy(), case["P"].copy()
    outs = garbage(15, 14)
    f = pg.lib.pgm_tree_likelihood
    args = [ctx.handle, 4, 8, 15, P(parent, C.c_uint32), 15, P(rows, C.c_int8), P(pi, C.c_double), P(Pm, C.c_double), 1,
            P(outs[0], C.c_double), P(outs[1], C.c_int32), P(outs[2], C.c_double), P(outs[3], C.c_double)]
    bad = []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 4, 6, 7, 8, 10, 11, 12, 13):                            # null pointers (d1, d2: the call asks for derivatives)
        call({k: None})
    for k, v in ((1, 0), (1, 65), (2, 1), (2, 0), (5, 0), (3, 8), (3, 7)):   # dim, nleaves < 2, ncols == 0, nnodes <= nleaves
        call({k: v})
    def with_parent(changes):
        p = parent.copy()
        for k, v in changes.items():
            p[k] = v
        call({4: P(p, C.c_uint32)})
        return p
    keep = [with_parent({8: 8}), with_parent({8: 3}), with_parent({9: 15}), with_parent({9: 0xFFFFFFFE}),   # a parent <= its child, >= nnodes
            with_parent({0: 3}),                                          # a leaf that is a parent
            with_parent({0: 9}),                                          # node 8 keeps one child
            with_parent({13: 0xFFFFFFFF})]                                # two roots
    for v in (4, -3, 127, -128):                                          # a row value outside -2 .. dim - 1
        r = rows.copy(); r[7, 14] = v
        call({6: P(r, C.c_int8)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(outs[0] == GARBAGE_F) and np.all(outs[1] == GARBAGE_I) and np.all(outs[2] == GARBAGE_F) and np.all(outs[3] == GARBAGE_F)
    assert len(keep) == 7
    # d1 and d2 may be null without derivatives, and the context is as good as before
    a = list(args); a[9] = 0; a[12] = None; a[13] = None
    a[8] = P(R.make_case(4, 15, "balanced8", False)["P"], C.c_double)
    assert f(*a) == 0
    assert R.same_bits(outs[0], case["want"]["site_l"]) and np.all(outs[2] == GARBAGE_F)
    assert f(*args) == 0
    assert R.same_bits(outs[2], case["want"]["d1"]) and R.same_bits(outs[3], case["want"]["d2"])
    assert pg.lib.pgm_treelik_last_kernel_ms(ctx.handle) > 0


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("ml_fams")
    aa = bu.aa_families(d)
    return dict(aa=[f for f in aa if f.endswith("_n24.fa")][0], aa5=[f for f in aa if f.endswith("_n5.fa")][0], dna=bu.dna_families(d), codon=bu.codon_families(d),
                hky=bu.hky_model(d))


def _both(exe, oracle_build, fa, tmp_path, opts, tag):
    """The product driver on the device path and the oracle driver (the host loop): both files, stdout, ml_lnl and ml_rounds."""
    got = TM.run_ml(exe, fa, tmp_path, "hip" + tag, opts, env=dict(os.environ, PGM_DEVICE_TREELIK="1"))
    ref = TM.run_ml(os.path.join(oracle_build, "pgmsa_oracle"), fa, tmp_path, "ref" + tag, opts)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert got.tree == ref.tree and got.sites == ref.sites and got.stdout == ref.stdout and len(got.tree) > 0 and len(got.sites) > 0
    for k in ("ml_lnl", "ml_lnl_start", "ml_rounds", "ml_evaluations"):
        assert got.stats[k] == ref.stats[k], k
    assert got.stats["ml_kernel_ms"] > 0 and ref.stats["ml_kernel_ms"] == 0 and "PGM_DEVICE_TREELIK" in got.stats["switches"]
    return got, ref


def test_driver_equals_the_oracle_driver_aa(exe, oracle_build, fams, tmp_path):
    got, _ = _both(exe, oracle_build, fams["aa"], tmp_path, ["-i", "0"], "aa")
    TM.check_files(got, "aa", R.shipped("wag.qmat"))
    host = TM.run_ml(exe, fams["aa"], tmp_path, "host", ["-i", "0"], env=dict(os.environ, PGM_HOST_TREELIK="1"))
    assert (host.tree, host.sites) == (got.tree, got.sites) and host.stats["ml_kernel_ms"] == 0
    _both(exe, oracle_build, fams["aa5"], tmp_path, ["-T", "-i", "0"], "aa5")   # (start characters; -T)


def test_driver_equals_the_oracle_driver_dna(exe, oracle_build, fams, tmp_path):
    fa = [f for f in fams["dna"] if len(R.read_fasta(f)) >= 3][0]
    _both(exe, oracle_build, fa, tmp_path, ["--dna", "--custom_model", fams["hky"]], "dna")


def test_driver_equals_the_oracle_driver_codon(exe, oracle_build, fams, tmp_path):
    _both(exe, oracle_build, fams["codon"][1], tmp_path, ["--codon", "--ml_rounds", "5"], "codon")


def test_driver_beside_bootstrap(exe, oracle_build, fams, tmp_path):
    bs = lambda tag: ["-i", "0", "--bootstrap", "4", "--bootstrap_out", str(tmp_path / tag)]
    env = dict(os.environ, PGM_DEVICE_TREELIK="1")
    got = TM.run_ml(exe, fams["aa"], tmp_path, "hip", bs("hip.bs"), env=env)
    ref = TM.run_ml(os.path.join(oracle_build, "pgmsa_oracle"), fams["aa"], tmp_path, "ref", bs("ref.bs"))
    assert (got.tree, got.sites, got.stdout) == (ref.tree, ref.sites, ref.stdout) and len(got.sites) > 0
    assert got.stats["ml_lnl"] == ref.stats["ml_lnl"] and got.stats["ml_rounds"] == ref.stats["ml_rounds"] and got.stats["ml_kernel_ms"] > 0
    assert open(str(tmp_path / "hip.bs")).read() == open(str(tmp_path / "ref.bs")).read()
    plain = bu.run(exe, ["--fasta"] + bs("plain.bs") + [fams["aa"]], env)
    assert open(str(tmp_path / "plain.bs")).read() == open(str(tmp_path / "hip.bs")).read() and plain.stdout == got.stdout   # unchanged by the flags
    alone = TM.run_ml(exe, fams["aa"], tmp_path, "alone", ["-i", "0"], env=env)
    assert (alone.tree, alone.sites) == (got.tree, got.sites) and got.stats["bootstrap_replicates"] == 4


def test_default_route_by_size(exe, fams, tmp_path):
    """Without a switch the host loop runs below kTreelikDeviceMin = 24 taxa and the device from there on; the same files either way."""
    small = TM.run_ml(exe, fams["aa5"], tmp_path, "small", ["-i", "0"])
    assert small.stats["ml_kernel_ms"] == 0 and small.stats["switches"] == ""
    forced = TM.run_ml(exe, fams["aa5"], tmp_path, "forced", ["-i", "0"], env=dict(os.environ, PGM_DEVICE_TREELIK="1"))
    assert forced.stats["ml_kernel_ms"] > 0 and (forced.tree, forced.sites) == (small.tree, small.sites)
    large = TM.run_ml(exe, fams["aa"], tmp_path, "large", ["-i", "0"])
    assert large.stats["ml_kernel_ms"] > 0 and large.stats["switches"] == ""
