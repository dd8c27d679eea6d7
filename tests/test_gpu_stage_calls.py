"""The call path the satellite C entries share (csrc/pgm_capi.hip: StageCall) and the context's table of scratch slots.

Every entry that goes through it — the distance entries, the context-profile batch, the profile merge, gap masks and gap parsimony,
the WLS pair sums, BioNJ, the agreement counts, the transfer entries, the tree likelihood — is called here with a smallest shape and
with a larger one, and every result is compared bit for bit with the same call on a fresh context: a slot two stages shared by
accident, a buffer that did not grow, a copy still in flight when a call returns would all change bits.  What the kernels compute
is checked by the stages' own test files, whose call helpers this file reuses.

A resident result (pgm_csprofile_create_batch_res, PGM_MERGE_RESIDENT) is a device address: it is read through a plain merge
whose nodes are the matrix's columns one by one (identity transition matrices), a function of nothing but the matrix."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

import bionj_ref as B
import mldist_general_ref as R
import test_gpu_bionj as TB
import test_gpu_mldist_general as TM
import test_gpu_reroot as TR
import test_gpu_taxa as TX
import test_gpu_topology as TT
import test_gpu_transfer as TG
import test_gpu_wls as TW
import topology_ref as T
import treelik_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K50 = os.path.join(ROOT, "tests", "golden", "K50.lib")
GAP = 0xFFFFFFFF
P = lambda a, t: a.ctypes.data_as(C.POINTER(t))


def pg():
    import prographmsa_amd
    return prographmsa_amd


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def on_fresh(call, *args):
    c = pg().Context(0)
    try:
        return call(c, *args)
    finally:
        c.close()


# ---- the distance entries ----------------------------------------------------------------------------------------------------------
def mldist(ctx, big, eigen, npairs=None):
    dim = 20 if big else 4
    npairs = (40 if big else 3) if npairs is None else npairs
    counts, gaps, seqlen, _ = R.eigen_pairs(dim, max(npairs, 1), 5)
    Q, V, Vi, sig = R.eigen_model(dim)
    m, keep = TM._model(Q, R.AA_PAR, 1, 0, eig=(V, Vi, sig) if eigen else None)
    rc, dist, var = TM._run(ctx, m, counts, gaps, seqlen, npairs)
    pg().check(rc)
    return [dist, var]


def prealigned(ctx, big, npairs=None):
    nrows, ncols = (8, 40) if big else (3, 5)
    rng = np.random.default_rng(nrows)
    rows = rng.integers(-1, 20, (nrows, ncols)).astype(np.int8)
    pi, pj = [np.ascontiguousarray(a, np.uint32) for a in np.triu_indices(nrows, 1)]
    npairs = (len(pi) if big else 3) if npairs is None else npairs
    counts = np.full(max(npairs, 1) * 400, -1, np.int32); gaps = np.full(max(npairs, 1), 77, np.uint32)
    pg().check(pg().lib.pgm_prealigned_counts_batch(ctx.handle, 20, nrows, ncols, P(rows, C.c_int8), npairs, P(pi, C.c_uint32), P(pj, C.c_uint32),
                                                    P(counts, C.c_int32), P(gaps, C.c_uint32)))
    return [counts, gaps]


def kmer(ctx, big, nseq=None):
    n, ncols = (9, 64) if big else (3, 16)
    nseq = n if nseq is None else nseq
    counts = np.random.default_rng(n).poisson(0.6, (n, ncols)).astype(np.int32)
    counts[:, 0] += 1
    out = np.full(n * n, -3.0)
    pg().check(pg().lib.pgm_kmer_cosine(ctx.handle, nseq, ncols, P(counts, C.c_int32), P(out, C.c_double)))
    return [out]


# ---- merged profiles, and the read of a resident matrix through them ---------------------------------------------------------------
def merge_jobs(D, shapes, seed):
    """Merge jobs of random graphs n1 x n2 and a random monotone walk through both (as tests/test_gpu_merge.py draws them)."""
    rng = np.random.default_rng(seed)
    jobs, keep = [], []
    for n1, n2 in shapes:
        g1, g2 = [np.asfortranarray(rng.dirichlet(np.ones(D), n).T) for n in (n1, n2)]
        P1, P2 = [np.asfortranarray(rng.dirichlet(np.ones(D) * 3, D)) for _ in range(2)]
        k1, k2, fl = [], [], []
        i1 = i2 = 0
        while i1 < n1 or i2 < n2:
            r = rng.random()
            if i1 < n1 and i2 < n2 and r < 0.6:
                k1.append(i1); k2.append(i2); fl.append(0); i1 += 1; i2 += 1
            elif i1 < n1 and (r < 0.8 or i2 >= n2):
                k1.append(i1); k2.append(GAP); fl.append(0); i1 += 1
            else:
                k1.append(GAP); k2.append(i2); fl.append(int(rng.random() < 0.5)); i2 += 1
        k1, k2, fl = np.array(k1, np.uint32), np.array(k2, np.uint32), np.array(fl, np.uint8)
        out = np.full(D * len(k1), np.nan)
        j = pg().pgm_merge_job()
        j.dim, j.n1, j.n2, j.nnodes = D, n1, n2, len(k1)
        j.sites1, j.sites2, j.P1, j.P2 = P(g1, C.c_double), P(g2, C.c_double), P(P1, C.c_double), P(P2, C.c_double)
        j.k1, j.k2, j.g2_with_P1, j.profiles = P(k1, C.c_uint32), P(k2, C.c_uint32), P(fl, C.c_uint8), P(out, C.c_double)
        jobs.append(j)
        keep.append((g1, g2, P1, P2, k1, k2, fl, out))
    return jobs, keep


def read_resident(ctx, D, dev, ncols):
    """The resident D x ncols matrices at the device addresses `dev`, as a plain merge returns their columns."""
    eye, other = np.asfortranarray(np.eye(D)), np.asfortranarray(np.full((D, 1), 1.0 / D))
    jobs, outs, keep = [], [], []
    for d, n in zip(dev, ncols):
        k1, k2, fl, out = np.arange(n, dtype=np.uint32), np.full(n, GAP, np.uint32), np.zeros(n, np.uint8), np.full(D * n, np.nan)
        j = pg().pgm_merge_job()
        j.dim, j.n1, j.n2, j.nnodes = D, n, 1, n
        j.sites1, j.sites2, j.P1, j.P2 = C.cast(d, C.POINTER(C.c_double)), P(other, C.c_double), P(eye, C.c_double), P(eye, C.c_double)
        j.k1, j.k2, j.g2_with_P1, j.profiles = P(k1, C.c_uint32), P(k2, C.c_uint32), P(fl, C.c_uint8), P(out, C.c_double)
        jobs.append(j); outs.append(out); keep.append((k1, k2, fl))
    pg().check(pg().lib.pgm_merge_profiles_batch(ctx.handle, len(jobs), (pg().pgm_merge_job * len(jobs))(*jobs)))
    return outs


def merge(ctx, big, resident, njobs=None):
    D = 4
    jobs, keep = merge_jobs(D, [(40, 50), (33, 21)] if big else [(3, 3)], 5)
    njobs = len(jobs) if njobs is None else njobs
    arr = (pg().pgm_merge_job * len(jobs))(*jobs)
    if not resident:
        pg().check(pg().lib.pgm_merge_profiles_batch(ctx.handle, njobs, arr))
        return [k[-1] for k in keep]
    dev = (C.POINTER(C.c_double) * len(jobs))()
    pg().check(pg().lib.pgm_merge_profiles_batch_ex(ctx.handle, njobs, arr, pg().PGM_MERGE_RESIDENT, dev))
    return read_resident(ctx, D, list(dev), [j.nnodes for j in jobs]) if njobs else []


# ---- context profiles from tests/golden/K50.lib ------------------------------------------------------------------------------------
def k50_library():
    """(K, ncols, lprofiles, centre, priors) of the golden library in the layout of pgm_csprofile_load (tests/test_gpu_nw_cs.py: _cs_case)."""
    blocks = open(K50).read().split("ContextProfile")[1:]
    K, prior, cols = len(blocks), [], []
    for b in blocks:
        lines = b.strip().split("\n")
        prior.append(float([l for l in lines if l.startswith("PRIOR")][0].split()[1]))
        cols.append([[int(v) for v in l.split()[1:]] for l in lines if l[:1].isdigit()])
    v = np.array(cols, np.float64)                      # K x ncols x 20: -1000 log2 p
    ncols = v.shape[1]
    w = 1.3 * 0.9 ** np.abs(np.arange(ncols) - ncols // 2)
    lp = np.zeros((K, ncols, 21))
    lp[:, :, :20] = -v / 1000.0 * math.log(2.0) * w[None, :, None]
    centre = 2.0 ** (-v[:, ncols // 2, :] / 1000.0)
    return K, ncols, [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (lp, centre, np.log(np.array(prior)))]


def csprofile(ctx, big, resident, nseq=None):
    K, ncols, (lpf, cf, prf) = k50_library()
    pg().check(pg().lib.pgm_csprofile_load(ctx.handle, K, ncols, P(lpf, C.c_double), P(cf, C.c_double), P(prf, C.c_double)))
    lens = [20, 0, 31, 40, 25] if big else [5, 9]
    rng = np.random.default_rng(len(lens))
    syms = rng.integers(0, 21, sum(lens)).astype(np.int8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    out_offs = np.concatenate([[0], np.cumsum([20 * (n + 2) for n in lens])]).astype(np.uint64)
    tau, pi, pu = rng.uniform(0.05, 0.9, len(lens)), rng.dirichlet(np.ones(20) * 5), np.ascontiguousarray(rng.dirichlet(np.ones(20), len(lens)).reshape(-1))
    nseq = len(lens) if nseq is None else nseq
    args = (ctx.handle, nseq, P(syms, C.c_int8), P(offs, C.c_uint32), P(tau, C.c_double), P(pi, C.c_double), P(pu, C.c_double))
    if not resident:
        out = np.full(int(out_offs[-1]), np.nan)
        pg().check(pg().lib.pgm_csprofile_create_batch(*args, P(out, C.c_double), P(out_offs, C.c_uint64)))
        return [out]
    dev = (C.POINTER(C.c_double) * len(lens))()
    pg().check(pg().lib.pgm_csprofile_create_batch_res(*args, dev))
    return read_resident(ctx, 20, list(dev), [n + 2 for n in lens]) if nseq else []


# ---- gap masks and gap parsimony ---------------------------------------------------------------------------------------------------
def gapmasks(ctx, big, njobs=None):
    rng = np.random.default_rng(3)
    jobs_in = [(20, 200, 300), (7, 64, 130), (33, 0, 70)] if big else [(2, 3, 5)]
    jobs = (pg().pgm_gapmask_job * len(jobs_in))()
    keep, outs = [], []
    for i, (nrows, nin, nout) in enumerate(jobs_in):
        child = rng.random((nrows, nin)) < 0.3
        mapping = np.full(nout, GAP, np.uint32)
        mapping[np.sort(rng.choice(nout, nin, replace=False))] = np.arange(1, nin + 1, dtype=np.uint32)
        src = TR.pack(child) if nin else np.zeros((nrows, 1), np.uint64)
        dst = np.full((nrows, (nout + 63) // 64), 0xDEAD, np.uint64)
        keep += [src, mapping]; outs.append(dst)
        jobs[i].src, jobs[i].mapping, jobs[i].dst = P(src, C.c_uint64), P(mapping, C.c_uint32), P(dst, C.c_uint64)
        jobs[i].nrows, jobs[i].ncols_in, jobs[i].ncols_out = nrows, nin, nout
    pg().check(pg().lib.pgm_gapmask_extend_batch(ctx.handle, len(jobs_in) if njobs is None else njobs, jobs))
    return outs


def parsimony(ctx, big, njobs=None):
    rng = np.random.default_rng(4)
    nl, ncols, ncand = (16, 200, 4) if big else (4, 10, 1)
    cands = [(rng.random((nl, ncols)) < 0.3, TR.random_topology(rng, nl)) for _ in range(ncand)]
    rc, scores = TR.run_parsimony(ctx, cands[:ncand if njobs is None else njobs])
    pg().check(rc)
    return [scores]


# ---- WLS pair sums, BioNJ ----------------------------------------------------------------------------------------------------------
def wls_jobs(n):
    rng = np.random.default_rng(n)
    return TW.make_matrices(rng, n), [TW.make_job(rng, n, K) + (K,) for K in ((4, 5, 4, 5, 5, 4) if n > 8 else (4, 5))]


def wls_sums(ctx, n):
    return [TW.run_kernel(ctx, pg(), wls_jobs(n)[1])]


def wls(ctx, big):
    n = 40 if big else 8
    TW.load(ctx, pg(), *wls_jobs(n)[0])
    return wls_sums(ctx, n)


def bionj(ctx, big, planned):
    n = 20 if big else 4
    D, V = B.matrices("random", n)
    j, f, launches = TT.device_solo(ctx, D, V, T.plan("random", n)) if planned else TB.device_solo(ctx, D, V)
    assert launches == (2 if planned else 3 * (n - 3))   # (two kernels for a plan of joins; sums, scan and join per free join)
    return [np.array(j), f]


# ---- agreement counts, transfer entries, tree likelihood ---------------------------------------------------------------------------
def agreement(ctx, big):
    nrep, n, ncols = (3, 10, 40) if big else (1, 2, 3)
    where = np.random.default_rng(n).integers(-1, 6, (nrep, n, ncols)).astype(np.int32)
    return list(ctx.msa_agreement(where, np.full((n, ncols), 0xDEADBEEF, np.uint32), np.full((n, n), 0xABCD1234, np.uint32)))


def transfer_sets(big):
    n, nref, counts = (70, 9, [5, 0, 12, 3]) if big else (4, 2, [1, 2])
    rng = random.Random(n)
    return n, TG.bit_sets(n, nref, rng, True), [TG.bit_sets(n, c, rng, False) for c in counts]


def transfer_min(ctx, big):
    return [TG.device_phi(ctx, *transfer_sets(big))]


def transfer_taxa(ctx, big):
    n, ref, reps = transfer_sets(big)
    return list(TX.device_taxa(ctx, n, ref, [1] * len(ref), reps))


def treelik(ctx, big, derivs):
    case = L.make_case(20, 33, "balanced8", derivs) if big else L.make_case(4, 1, "three", derivs)
    nedges, ncols = len(case["parent"]) - 1, case["rows"].shape[1]
    return list(ctx.tree_likelihood(case["dim"], case["parent"], case["rows"], case["pi"], case["P"], derivs=derivs,
                                    out=(np.full(ncols, -7.25e77), np.full(ncols, -77777, np.int32), np.full(nedges, -7.25e77), np.full(nedges, -7.25e77))))


# every converted entry: name -> (call(ctx, big), the accessor of its stage's timer, its empty call or None where it accepts none)
ENTRIES = {
    "mldist_eigen": (lambda c, big: mldist(c, big, True), "pgm_dist_last_kernel_ms", lambda c: mldist(c, False, True, 0)),
    "mldist_general": (lambda c, big: mldist(c, big, False), "pgm_dist_last_kernel_ms", lambda c: mldist(c, False, False, 0)),
    "prealigned": (prealigned, "pgm_dist_last_kernel_ms", lambda c: prealigned(c, False, 0)),
    "kmer_cosine": (kmer, "pgm_dist_last_kernel_ms", lambda c: kmer(c, False, 0)),
    "csprofile": (lambda c, big: csprofile(c, big, False), "pgm_csprofile_last_kernel_ms", lambda c: csprofile(c, False, False, 0)),
    "csprofile_resident": (lambda c, big: csprofile(c, big, True), "pgm_csprofile_last_kernel_ms", lambda c: csprofile(c, False, True, 0)),
    "merge": (lambda c, big: merge(c, big, False), "pgm_merge_last_kernel_ms", lambda c: merge(c, False, False, 0)),
    "merge_resident": (lambda c, big: merge(c, big, True), "pgm_merge_last_kernel_ms", lambda c: merge(c, False, True, 0)),
    "gapmasks": (gapmasks, "pgm_parsimony_last_kernel_ms", lambda c: gapmasks(c, False, 0)),
    "parsimony": (parsimony, "pgm_parsimony_last_kernel_ms", lambda c: parsimony(c, False, 0)),
    "wls": (wls, "pgm_wls_last_kernel_ms", lambda c: TW.run_kernel(c, pg(), [])),
    "bionj": (lambda c, big: bionj(c, big, False), "pgm_bionj_last_kernel_ms", None),
    "bionj_planned": (lambda c, big: bionj(c, big, True), "pgm_bionj_last_kernel_ms", None),
    "agreement": (agreement, "pgm_agreement_last_kernel_ms", None),
    "transfer_min": (transfer_min, "pgm_transfer_last_kernel_ms", None),
    "transfer_taxa": (transfer_taxa, "pgm_transfer_last_kernel_ms", None),
    "treelik": (lambda c, big: treelik(c, big, True), "pgm_treelik_last_kernel_ms", None),
    "treelik_no_derivs": (lambda c, big: treelik(c, big, False), "pgm_treelik_last_kernel_ms", None),
}


def test_slots_do_not_collide(ctx):
    """The matrices of pgm_wls_load stay in their slot while every other entry runs on the context: the pair sums of a call behind
    all of them, without another load, have the bits of the call before; and every entry in between gives what it gives alone."""
    TW.load(ctx, pg(), *wls_jobs(8)[0])
    first = wls_sums(ctx, 8)
    assert same(first, on_fresh(wls, False))
    for name, (call, _, _) in ENTRIES.items():
        if name != "wls":
            assert same(call(ctx, False), on_fresh(call, False)), name
    assert same(wls_sums(ctx, 8), first)
    assert pg().lib.pgm_wls_last_launches(ctx.handle) == 2


@pytest.mark.parametrize("name", list(ENTRIES))
def test_grow_shrink_grow(name):
    """Small, then more than 1.25 times larger in every buffer (every scratch slot of the entry is replaced: a slot grows to
    bytes + bytes / 4), then small again, on a context of the test's own."""
    call = ENTRIES[name][0]
    one = pg().Context(0)
    try:
        small, large, again = call(one, False), call(one, True), call(one, False)
    finally:
        one.close()
    assert same(small, on_fresh(call, False)), name
    assert same(large, on_fresh(call, True)), name
    assert same(again, small), name


@pytest.mark.parametrize("name", list(ENTRIES))
def test_timers_and_counters(ctx, name):
    call, ms, empty = ENTRIES[name]
    ms = getattr(pg().lib, ms)
    call(ctx, False)
    assert ms(ctx.handle) > 0, name
    if name == "wls":
        assert pg().lib.pgm_wls_last_launches(ctx.handle) == 2
    if empty is not None:
        empty(ctx)
        assert ms(ctx.handle) == 0, name
        if name == "wls":
            assert pg().lib.pgm_wls_last_launches(ctx.handle) == 0
