"""`--bootstrap` on the MI355X: pgm_prealigned_counts_resampled against pgm_prealigned_counts_batch on the host-gathered matrix of
every replicate (exact integers), and the product driver against the CPU oracle driver, byte for byte.  Every driver run is a child
process under a time limit of its own."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu

pytestmark = pytest.mark.gpu
P = lambda a, t: a.ctypes.data_as(C.POINTER(t))


def _rows(rng, dim, n, L):
    r = rng.integers(0, dim, (n, L)).astype(np.int8)
    r[rng.random((n, L)) < 0.3] = -1
    r[rng.random((n, L)) < 0.04] = -2
    return r


def _cols(rng, kind, L):
    if kind == "identity":
        return np.arange(L, dtype=np.uint32)
    if kind == "reversal":
        return np.arange(L, dtype=np.uint32)[::-1].copy()
    if kind == "repeated":
        return np.full(L, int(rng.integers(0, L)), np.uint32)
    return rng.integers(0, L, L).astype(np.uint32)


def _reference(pg, ctx, dim, rows, cols, pi, pj):
    """pgm_prealigned_counts_batch on the gathered matrix of every replicate (the per-family entry takes 20 to 64 states: a smaller
    matrix is the corner of its 20 x 20)."""
    Dk = max(dim, 20)
    counts, gaps = [], []
    for c in cols:
        m = np.ascontiguousarray(rows[:, c])
        cc = np.zeros(len(pi) * Dk * Dk, np.int32)
        g = np.zeros(len(pi), np.uint32)
        pg.check(pg.lib.pgm_prealigned_counts_batch(ctx.handle, Dk, m.shape[0], m.shape[1], P(m, C.c_int8), len(pi), P(pi, C.c_uint32), P(pj, C.c_uint32),
                                                    P(cc, C.c_int32), P(g, C.c_uint32)))
        counts.append(cc.reshape(len(pi), Dk, Dk)[:, :dim, :dim].reshape(len(pi), dim * dim))
        gaps.append(g)
    return np.array(counts), np.array(gaps)


def _all_pairs(n):
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)


@pytest.mark.parametrize("dim", [4, 20, 61])
def test_resampled_counts_equal_the_gathered_matrix(ctx, dim):
    import prographmsa_amd as pg
    rng = np.random.default_rng(4100 + dim)
    moved = 0
    for L in (1, 63, 64, 65, 300):
        for n in (2, 3, 24):
            rows = _rows(rng, dim, n, L)
            pi, pj = _all_pairs(n)
            sets = [["identity"], ["reversal"], ["repeated"], ["random"], ["reversal", "repeated", "random"], ["random", "identity", "random"]]
            for kinds in sets:   # nrep 1 and 3
                cols = np.array([_cols(rng, k, L) for k in kinds], np.uint32)
                counts, gaps = ctx.prealigned_counts_resampled(dim, rows, cols, pi, pj)
                rc, rg = _reference(pg, ctx, dim, rows, cols, pi, pj)
                assert counts.shape == rc.shape and np.array_equal(counts, rc), (L, n, kinds)
                assert np.array_equal(gaps, rg), (L, n, kinds)
                if kinds == ["reversal"] or kinds == ["repeated"]:   # (the gap openings are the gathered matrix's, not the stored one's)
                    ident = _reference(pg, ctx, dim, rows, np.arange(L, dtype=np.uint32)[None, :], pi, pj)[1]
                    moved += int(not np.array_equal(ident, rg))
    assert moved > 0


def test_pair_lists_and_buffer_reuse(ctx):
    import prographmsa_amd as pg
    rng = np.random.default_rng(77)
    # a pair list with a repeated pair, a pair in both orders and a row with itself
    rows = _rows(rng, 20, 5, 130)
    pi = np.array([0, 3, 0, 4, 2, 0], np.uint32)
    pj = np.array([1, 4, 1, 3, 2, 1], np.uint32)
    cols = np.array([_cols(rng, k, 130) for k in ("random", "reversal", "random")], np.uint32)
    counts, gaps = ctx.prealigned_counts_resampled(20, rows, cols, pi, pj)
    rc, rg = _reference(pg, ctx, 20, rows, cols, pi, pj)
    assert np.array_equal(counts, rc) and np.array_equal(gaps, rg)
    assert np.array_equal(counts[:, 0], counts[:, 2]) and np.array_equal(counts[:, 0], counts[:, 5])
    # calls of different shapes on one context: large, small, large again, with more replicates than the first
    for n, L, nrep in ((24, 700, 5), (2, 3, 1), (9, 257, 11)):
        rows = _rows(rng, 20, n, L)
        pi, pj = _all_pairs(n)
        cols = rng.integers(0, L, (nrep, L)).astype(np.uint32)
        counts, gaps = ctx.prealigned_counts_resampled(20, rows, cols, pi, pj)
        rc, rg = _reference(pg, ctx, 20, rows, cols, pi, pj)
        assert np.array_equal(counts, rc) and np.array_equal(gaps, rg), (n, L, nrep)


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    rng = np.random.default_rng(5)
    n, L, nrep = 3, 40, 2
    rows = _rows(rng, 20, n, L)
    cols = rng.integers(0, L, (nrep, L)).astype(np.uint32)
    pi, pj = _all_pairs(n)
    counts = np.full(nrep * len(pi) * 400, -7, np.int32)
    gaps = np.full(nrep * len(pi), 12345, np.uint32)
    f = pg.lib.pgm_prealigned_counts_resampled
    args = [ctx.handle, 20, n, L, P(rows, C.c_int8), nrep, P(cols, C.c_uint32), len(pi), P(pi, C.c_uint32), P(pj, C.c_uint32), P(counts, C.c_int32), P(gaps, C.c_uint32)]
    bad = []
    for k in (0, 4, 6, 8, 9, 10, 11):          # null pointers
        a = list(args); a[k] = None
        bad.append(f(*a))
    for k, v in ((5, 0), (2, 1), (2, 0), (3, 0), (1, 0), (1, 65)):   # nrep == 0, nrows < 2, ncols == 0, dim outside 1..64
        a = list(args); a[k] = v
        bad.append(f(*a))
    far = pj.copy(); far[1] = n                 # a pair index >= nrows
    a = list(args); a[9] = P(far, C.c_uint32)
    bad.append(f(*a))
    far = pi.copy(); far[0] = 0xFFFFFFFF
    a = list(args); a[8] = P(far, C.c_uint32)
    bad.append(f(*a))
    out = cols.copy(); out[1, L - 1] = L        # a cols entry >= ncols
    a = list(args); a[6] = P(out, C.c_uint32)
    bad.append(f(*a))
    assert all(rc == pg.PGM_ERR_INVALID for rc in bad), bad
    assert np.all(counts == -7) and np.all(gaps == 12345)   # nothing was launched
    assert f(*args) == 0                        # the context is as good as before
    rc, rg = _reference(pg, ctx, 20, rows, cols, pi, pj)
    assert np.array_equal(counts.reshape(rc.shape), rc) and np.array_equal(gaps.reshape(rg.shape), rg)


# ---- the driver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    all_fams = bu.aa_families(tmp_path_factory.mktemp("boot_fams"))
    return [next(f for f in all_fams if f.endswith("_n%d.fa" % n)) for n in (5, 13, 24)]


def _bootstrap(exe, fa, out, opts, env=None):
    r = bu.run(exe, ["--fasta", "--stats", "--bootstrap", "8", "--bootstrap_out", out] + list(opts) + [fa], env)
    with open(out) as f:
        return f.read(), r.stdout, bu.stats_of(r.stderr)


@pytest.mark.parametrize("flow", ["default", "mldist", "device_bionj"])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, flow):
    opts = ["-m"] if flow == "mldist" else []
    env = dict(os.environ, PGM_DEVICE_BIONJ="1") if flow == "device_bionj" else None
    for k, fa in enumerate(fams):
        got, out, st = _bootstrap(exe, fa, str(tmp_path / ("hip%d.nwk" % k)), opts, env)
        ref, ref_out, ref_st = _bootstrap(os.path.join(oracle_build, "pgmsa_oracle"), fa, str(tmp_path / ("ref%d.nwk" % k)), opts)
        assert st["backend"] == "hip" and ref_st["backend"] == "oracle"
        assert got == ref and len(got) > 0 and out == ref_out
        assert st["bootstrap_replicates"] == 8 and st["bootstrap_counts_calls"] == 1
        if flow == "device_bionj":
            assert st["bionj_device_calls"] >= 2   # (the tree of the alignment and the replicates' call)
