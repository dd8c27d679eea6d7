"""Weighted least-squares refinement on the MI355X: the subtree pair-sum kernels (pgm_wls_pair_sums_batch) against a
math.fsum statement and against a numpy statement of their documented summation order, and `pgmsa -W / -WW` against the
CPU oracle driver, whose pair sums are the host's statement of that order."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import gen
import test_cpu_wls as T

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def _P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def make_matrices(rng, n):
    D = rng.uniform(0.0, 2.0, (n, n))
    D = (D + D.T) / 2
    W = 1.0 / rng.uniform(1e-3, 1.0, (n, n))
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(W, np.inf)   # (1 / variance of the diagonal, as the refinement loads it; never part of a pair)
    return np.ascontiguousarray(D), np.ascontiguousarray(W)


def make_job(rng, n, K, empty=None):
    lab = rng.integers(-1, K, n).astype(np.int8)
    if n >= K:
        lab[rng.permutation(n)[:K]] = np.arange(K)   # (every subtree non-empty unless asked otherwise)
    if empty is not None:
        lab[lab == empty] = -1
    off = np.where(lab >= 0, rng.uniform(0.0, 0.5, n), 0.0)
    return lab, np.ascontiguousarray(off)


def pairs(K):
    return [(p, q) for p in range(K) for q in range(p + 1, K)]


def run_kernel(ctx, pg, jobs):
    arr = (pg.pgm_wls_job * len(jobs))()
    for i, (lab, off, K) in enumerate(jobs):
        arr[i].label, arr[i].offset, arr[i].nsub = _P(lab, C.c_int8), _P(off, C.c_double), K
    out = np.full(len(jobs) * 20, np.nan)
    pg.check(pg.lib.pgm_wls_pair_sums_batch(ctx.handle, len(jobs), arr, _P(out, C.c_double)), "pgm_wls_pair_sums_batch")
    return out.reshape(len(jobs), 20)


def load(ctx, pg, D, W):
    pg.check(pg.lib.pgm_wls_load(ctx.handle, D.shape[0], _P(D, C.c_double), _P(W, C.c_double)), "pgm_wls_load")


def fsum_statement(D, W, lab, off, K):
    """Exact-rounded sums of the reference's terms W(k,l) * ((D(k,l) - a_k) - b_l), k in p, l in q; and the bound on each."""
    S, Wt, bound = np.zeros(10), np.zeros(10), np.zeros(10)
    for s, (p, q) in enumerate(pairs(K)):
        kp, lq = np.flatnonzero(lab == p), np.flatnonzero(lab == q)
        w = W[np.ix_(kp, lq)]
        t = w * ((D[np.ix_(kp, lq)] - off[kp][:, None]) - off[lq][None, :])
        S[s], Wt[s] = math.fsum(t.ravel()), math.fsum(w.ravel())
        bound[s] = float(np.abs(t).sum())
    return S, Wt, bound


def butterfly(v):
    v = v.copy()
    m = 32
    while m >= 1:
        v[..., :m] = v[..., :m] + v[..., m:2 * m]
        m //= 2
    return v[..., 0]


def order_statement(D, W, lab, off, K):
    """The kernels' summation order (csrc/pgm_wls_kernels.h) in numpy: the same bits."""
    n = len(lab)
    R = np.zeros((n, 2, 4))
    labk = lab.astype(np.int64)
    for j in range(4):
        S, Wl = np.zeros((n, 64)), np.zeros((n, 64))
        for c in range(0, n, 64):
            sl = slice(c, min(c + 64, n))
            m = sl.stop - sl.start
            msk = ((labk[sl][None, :] - labk[:, None] - 1) == j) & (labk[:, None] >= 0)
            with np.errstate(invalid="ignore"):
                t = W[:, sl] * ((D[:, sl] - off[:, None]) - off[None, sl])
            S[:, :m] = np.where(msk, S[:, :m] + t, S[:, :m])
            Wl[:, :m] = np.where(msk, Wl[:, :m] + W[:, sl], Wl[:, :m])
        R[:, 0, j], R[:, 1, j] = butterfly(S), butterfly(Wl)
    nb = (n + 15) // 16
    part = np.zeros((nb, 20))
    for b in range(nb):
        acc = np.zeros((4, 20))
        for v in range(4):
            for i in range(4):
                k = b * 16 + v + 4 * i
                if k >= n:
                    break
                p = int(lab[k])
                if p < 0 or p >= K - 1:
                    continue
                base = p * K - p * (p + 1) // 2
                for jj in range(K - 1 - p):
                    acc[v, base + jj] += R[k, 0, jj]
                    acc[v, 10 + base + jj] += R[k, 1, jj]
        part[b] = (acc[0] + acc[1]) + (acc[2] + acc[3])
    lanes = np.zeros((20, 64))
    for b in range(nb):
        lanes[:, b % 64] += part[b]
    return butterfly(lanes)


def check_job(out, D, W, lab, off, K, exact=True):
    S, Wt, bound = fsum_statement(D, W, lab, off, K)
    n = len(lab)
    P = len(pairs(K))
    tol = (n / 32 + 32) * EPS   # depth of the summation tree, in units of the terms' magnitude
    assert np.all(np.abs(out[:P] - S[:P]) <= tol * bound[:P]), (out[:P], S[:P])
    assert np.all(np.abs(out[10:10 + P] - Wt[:P]) <= tol * Wt[:P]), (out[10:10 + P], Wt[:P])
    assert np.all(out[P:10] == 0) and np.all(out[10 + P:] == 0)
    if exact:
        assert np.array_equal(out, order_statement(D, W, lab, off, K))


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 257, 1024])
def test_pair_sums_kernel(ctx, n):
    import prographmsa_amd as pg
    rng = np.random.default_rng(n)
    D, W = make_matrices(rng, n)
    load(ctx, pg, D, W)
    jobs = [make_job(rng, n, K) + (K,) for K in (4, 5, 4, 5)]
    jobs.append(make_job(rng, n, 5, empty=2) + (5,))   # an empty subtree: its pairs are exact zeros
    out = run_kernel(ctx, pg, jobs)
    assert pg.lib.pgm_wls_last_launches(ctx.handle) == 2
    for (lab, off, K), o in zip(jobs, out):
        check_job(o, D, W, lab, off, K, exact=n <= 257)
    empty = [s for s, (p, q) in enumerate(pairs(5)) if 2 in (p, q)]
    assert np.all(out[-1][empty] == 0) and np.all(out[-1][[10 + s for s in empty]] == 0)
    for i, job in enumerate(jobs):   # one job per call gives the same bits as the batch
        assert np.array_equal(run_kernel(ctx, pg, [job])[0], out[i])


@pytest.mark.parametrize("n", [65, 1024])
def test_pair_sums_kernel_batch_of_all_edges(ctx, n):
    """The support pass's shape: n - 3 jobs in one call."""
    import prographmsa_amd as pg
    rng = np.random.default_rng(100 + n)
    D, W = make_matrices(rng, n)
    load(ctx, pg, D, W)
    jobs = [make_job(rng, n, 4) + (4,) for _ in range(n - 3)]
    out = run_kernel(ctx, pg, jobs)
    for i in sorted(set([0, 1, n // 2, n - 4] + list(rng.integers(0, n - 3, 4)))):
        check_job(out[i], D, W, *jobs[i], exact=(n <= 65 or i == 0))
        assert np.array_equal(run_kernel(ctx, pg, [jobs[i]])[0], out[i])


def test_pair_sums_rejects_bad_input(ctx):
    import prographmsa_amd as pg
    rng = np.random.default_rng(3)
    fresh = pg.Context(0)
    lab, off = make_job(rng, 8, 4)
    arr = (pg.pgm_wls_job * 1)()
    arr[0].label, arr[0].offset, arr[0].nsub = _P(lab, C.c_int8), _P(off, C.c_double), 4
    out = np.zeros(20)
    assert pg.lib.pgm_wls_pair_sums_batch(fresh.handle, 1, arr, _P(out, C.c_double)) == pg.PGM_ERR_INVALID   # nothing loaded
    fresh.close()
    D, W = make_matrices(rng, 8)
    one = np.zeros(1)
    assert pg.lib.pgm_wls_load(ctx.handle, 1, _P(one, C.c_double), _P(one, C.c_double)) == pg.PGM_ERR_INVALID
    assert pg.lib.pgm_wls_load(ctx.handle, 32769, _P(one, C.c_double), _P(one, C.c_double)) == pg.PGM_ERR_INVALID
    assert pg.lib.pgm_wls_load(ctx.handle, 8, None, _P(W, C.c_double)) == pg.PGM_ERR_INVALID
    load(ctx, pg, D, W)
    for nsub in (0, 3, 6):
        arr[0].nsub = nsub
        assert pg.lib.pgm_wls_pair_sums_batch(ctx.handle, 1, arr, _P(out, C.c_double)) == pg.PGM_ERR_INVALID
    for bad, nsub in ((4, 4), (5, 5), (-2, 4)):
        l2 = lab.copy()
        l2[3] = bad
        arr[0].label, arr[0].nsub = _P(l2, C.c_int8), nsub
        assert pg.lib.pgm_wls_pair_sums_batch(ctx.handle, 1, arr, _P(out, C.c_double)) == pg.PGM_ERR_INVALID
    arr[0].label, arr[0].nsub = None, 4
    assert pg.lib.pgm_wls_pair_sums_batch(ctx.handle, 1, arr, _P(out, C.c_double)) == pg.PGM_ERR_INVALID
    assert pg.lib.pgm_wls_pair_sums_batch(ctx.handle, 1, None, _P(out, C.c_double)) == pg.PGM_ERR_INVALID
    arr[0].label = _P(lab, C.c_int8)
    assert pg.lib.pgm_wls_pair_sums_batch(ctx.handle, 1, arr, _P(out, C.c_double)) == pg.PGM_OK


def _both(oracle_build, args):
    import prographmsa_amd as pg
    out = []
    for exe in (pg.PGMSA_PATH, os.path.join(oracle_build, "pgmsa_oracle")):
        r = subprocess.run([exe] + args + ["--stats"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (exe, r.stderr)
        out.append((r.stdout, json.loads(r.stderr.strip().splitlines()[-1])))
    return out


@pytest.mark.parametrize("idx", range(len(T.WLS["trees"])), ids=lambda i: "n%d" % T.WLS["trees"][i]["n"])
def test_pgmsa_wls_trees_equal_oracle(oracle_build, tmp_path, idx):
    rec = T.WLS["trees"][idx]
    fa = T.write_family(tmp_path, rec)
    for flag in ("-W", "-WW"):
        (prod, st), (orac, _) = _both(oracle_build, ["-T", "-i", "0", "-a", flag, fa])
        assert prod == orac
        assert st["wls_launches"] == 2 * st["wls_batches"] > 0


@pytest.mark.parametrize("idx", range(len(T.WLS["fasta"])), ids=lambda i: "n%d" % T.WLS["fasta"][i]["n"])
def test_pgmsa_wls_fasta_equals_oracle(oracle_build, tmp_path, idx):
    rec = T.WLS["fasta"][idx]
    fa = T.write_family(tmp_path, rec)
    for flag in ("-W", "-WW"):
        (prod, _), (orac, _) = _both(oracle_build, ["--fasta", "-a", "-m", flag, fa])
        assert prod == orac


def test_pgmsa_wls_1024_taxa_equals_oracle(oracle_build, tmp_path):
    fa = tmp_path / "big.fa"
    fa.write_text(gen.fasta(gen.gen(1024, 300, 11)))
    (prod, st), (orac, _) = _both(oracle_build, ["-T", "-i", "0", "-W", str(fa)])
    assert prod == orac
    assert st["wls_quartets"] > 1021 and st["wls_sweeps"] >= 2
