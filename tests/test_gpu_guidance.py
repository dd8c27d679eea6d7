"""`--guidance` on the MI355X: pgm_msa_agreement against a brute-force numpy compare (exact integers) over the shapes around the
kernels' tiles (64 rows, chunks of 32 columns) and the contents that can go wrong (gaps, all-gap rows and columns, the exact
maximum, no agreement at all, column values up to 2^31 - 1, a reduced axis long enough for the grid-stride loops), the refusal of
sizes whose sums do not fit 32 bits, and the product driver against the CPU oracle driver, byte for byte.  Every driver run is a
child process under a time limit of its own."""
import os

import numpy as np
import pytest

import guidance_ref as G

pytestmark = pytest.mark.gpu
T, K = 64, 32   # PGM_AGREE_T, PGM_AGREE_K of csrc/pgm_agreement_kernels.h


def _random_where(rng, nrep, n, L, gaps=0.3, hi=40):
    w = rng.integers(0, hi, (nrep, n, L)).astype(np.int32)
    w[rng.random((nrep, n, L)) < gaps] = -1
    return w


def _check(ctx, where, what):
    where = np.ascontiguousarray(where, np.int32)
    nrep, n, L = where.shape
    res = np.full((n, L), 0xDEADBEEF, np.uint32)      # garbage that must be overwritten
    pair = np.full((n, n), 0xABCD1234, np.uint32)
    ctx.msa_agreement(where, res, pair)
    want_res, want_pair = G.agreement(where)
    assert np.array_equal(res.astype(np.int64), want_res), what
    assert np.array_equal(pair.astype(np.int64), want_pair), what
    assert np.array_equal(pair, pair.T) and not pair.diagonal().any(), what
    assert int(res.sum(dtype=np.int64)) == int(pair.sum(dtype=np.int64)), what
    return res, pair


@pytest.mark.parametrize("nrep", [1, 2, 7])
def test_agreement_equals_numpy_over_the_tile_shapes(ctx, nrep):
    rng = np.random.default_rng(900 + nrep)
    for n in (1, 2, 3, T - 1, T, T + 1, 2 * T + 1):
        for L in (1, K - 1, K, K + 1, 300):
            # few distinct values: many agreements; 30 % gaps
            _check(ctx, _random_where(rng, nrep, n, L, hi=int(rng.integers(2, 12))), (nrep, n, L))


def test_agreement_contents(ctx):
    rng = np.random.default_rng(17)
    nrep, n, L = 3, T + 1, 2 * K + 6
    # all-gap rows and all-gap columns among random values
    w = _random_where(rng, nrep, n, L, hi=5)
    w[:, 0, :] = -1; w[:, T - 1, :] = -1; w[:, T, :] = -1
    w[:, :, 0] = -1; w[:, :, K] = -1; w[:, :, L - 1] = -1
    w[1, 5, :] = -1                                    # (and a row that is all gaps in one replicate only)
    res, pair = _check(ctx, w, "all-gap rows and columns")
    assert not res[0].any() and not res[:, K].any() and not pair[T].any() and not pair[:, 0].any()
    # every value -1: two gaps never hit
    res, pair = _check(ctx, np.full((nrep, n, L), -1, np.int32), "all gaps")
    assert not res.any() and not pair.any()
    # other negative values are gaps too
    res, pair = _check(ctx, np.full((nrep, n, L), -2, np.int32), "all -2")
    assert not res.any() and not pair.any()
    # where[r][i][c] = c: the exact maximum
    w = np.broadcast_to(np.arange(L, dtype=np.int32), (nrep, n, L))
    res, pair = _check(ctx, w, "maximum")
    assert np.all(res == nrep * (n - 1)) and np.all(pair + np.eye(n, dtype=np.uint32) * (nrep * L) == nrep * L)
    # values unique per row: nothing agrees
    w = (np.arange(n, dtype=np.int32)[None, :, None] * 1000 + np.arange(L, dtype=np.int32)[None, None, :]) * np.ones((nrep, 1, 1), np.int32)
    res, pair = _check(ctx, w, "unique per row")
    assert not res.any() and not pair.any()
    # column values up to 2^31 - 1
    big = np.array([2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 0], np.int32)
    w = big[rng.integers(0, 4, (nrep, n, L))]
    w[rng.random((nrep, n, L)) < 0.2] = -1
    _check(ctx, w, "large values")


def test_agreement_long_reduced_axis_and_repeat_calls(ctx):
    """More (replicate, column chunk) pairs and more replicates than the grids hold workgroups along the reduced axis (about four
    workgroups per CU in all): the round-robin loops of both kernels run more than once.  Two calls give identical results, and a
    small call after a large one on the same context sees nothing of it."""
    rng = np.random.default_rng(23)
    w = _random_where(rng, 150, 3, 2000, hi=3)
    res, pair = _check(ctx, w, "long axis")
    res2, pair2 = _check(ctx, w, "long axis again")
    assert np.array_equal(res, res2) and np.array_equal(pair, pair2)
    _check(ctx, _random_where(rng, 1, 2, 3), "small after large")
    got = ctx.msa_agreement(w)                                              # (outputs allocated by the binding)
    assert np.array_equal(got[0], res) and np.array_equal(got[1], pair)


def test_agreement_refuses_sums_beyond_32_bits(ctx):
    import prographmsa_amd as pg
    f = pg.lib.pgm_msa_agreement
    # sizes only: the refusal comes before any buffer is touched
    assert f(ctx.handle, 2, 2 ** 31, 2, None, None, None) == pg.PGM_ERR_INVALID          # nrep * ncols = 2^32
    assert "32 bits" in pg.lib.pgm_last_error().decode()
    assert f(ctx.handle, 65537, 1, 65536, None, None, None) == pg.PGM_ERR_INVALID        # nrep * (nrows - 1) = 2^32
    assert "32 bits" in pg.lib.pgm_last_error().decode()
    for shape in ((0, 5, 1), (5, 0, 1), (5, 5, 0)):
        assert f(ctx.handle, shape[0], shape[1], shape[2], None, None, None) == pg.PGM_ERR_INVALID
    assert f(ctx.handle, 2, 2, 2, None, None, None) == pg.PGM_ERR_INVALID                # null pointers
    _check(ctx, _random_where(np.random.default_rng(1), 2, 5, 40), "after the refusals")  # the context is as good as before


# ---- the driver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return G.families(tmp_path_factory.mktemp("guidance_fams"))


@pytest.mark.parametrize("kind", G.KINDS)
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, kind):
    fa, opts = fams[kind]
    got = G.guidance(exe, fa, tmp_path, "hip", 6, opts=opts)
    ref = G.guidance(os.path.join(oracle_build, "pgmsa_oracle"), fa, tmp_path, "ref", 6, opts=opts)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert got.stdout == ref.stdout and len(got.out) > 0
    assert got.out == ref.out and got.res == ref.res
    assert got.trees == ref.trees and got.alns == ref.alns
    assert got.stats["guidance_replicates"] == 6 and got.stats["guidance_agreement_calls"] >= 1


def test_driver_groups_equal_the_oracle_driver(exe, oracle_build, fams, tmp_path):
    """--batch_cells small enough for several forest groups, hence several agreement calls whose counts the host adds."""
    fa, opts = fams["aa"]
    cells = ["--batch_cells", "250000"]
    got = G.guidance(exe, fa, tmp_path, "hipg", 6, opts=opts + cells, dump=False)
    ref = G.guidance(os.path.join(oracle_build, "pgmsa_oracle"), fa, tmp_path, "refg", 6, opts=opts, dump=False)
    assert got.stats["backend"] == "hip"
    assert 1 < got.stats["guidance_passes"] <= 6 and 1 < got.stats["guidance_agreement_calls"] <= 6
    assert ref.stats["guidance_passes"] == 1
    assert got.out == ref.out and got.res == ref.res and got.stdout == ref.stdout
