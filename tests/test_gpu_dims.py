"""GPU parity at every alphabet size the C ABI accepts, not only the product's 20 (amino acids) and 61 (codons).

The oracle (oracle/pgm_oracle.c) is written for any D, the packets of four of the denominators and their D % 4 tail included.
The sizes are those where the kernels branch: 1-5 (DNA is 4), 19-23 on both sides of the 20 / 64 padding of the converted
profiles, 32 / 33 (the merge kernel's 32 / 64 padding), 60-64 (the lean kernel's class header and LDS score table at their
largest).  Jobs of different sizes in one batch share the batch's padded stride (pgm_align_batch_create_res); every entry point
refuses a size just outside its range and the context stays usable."""
import ctypes as C

import numpy as np
import pytest

import align_cases as A
from test_gpu_align import FAMILIES, _cmp_job, _jobs

pytestmark = pytest.mark.gpu

DIMS, SIZES = A.DIMS, A.DIM_SIZES
# pure chains, one-hot rows (in the product form: two sequence graphs, the lean kernel's score table), chains with edge costs,
# skip edges (wide workers and crit3 jobs), dense extras (crit3 jobs: no node of them is generic), far edges, heavy-tailed edges
# (MODE 2 long entries, generic columns); align_cases.DIMS_CLAIMS holds each to it
SWEEP_FAMILIES = {name: FAMILIES[fi] for name, fi in A.SWEEP_FAMILIES.items()}
# the critical-path kernel's shape: 21 bands, every predecessor near or in the on-chip history (a small batch: pgm_crit_kernel)
CRIT = A.DIM_CRIT
P = lambda a, t: a.ctypes.data_as(C.POINTER(t))


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _same(r, ref):
    assert r["status"] == ref["status"] == 0 and r["n_tr_indels"] == ref["n_tr_indels"]
    assert _bits(r["score"]) == _bits(ref["score"])
    assert np.array_equal(r["map1"], ref["map1"]) and np.array_equal(r["map2"], ref["map2"])


def _sequence_pair(job):
    """Both graphs are plain chains whose every column is one-hot, uniform 1 / D or empty (as floats): the product form of the
    batch then looks the job's scores up in its class table (pgm_classify_kernel, pgm_lean_kernel)."""
    def chain(g):
        return (g.r_col is None and g.e_rowptr[0] == 0 and g.e_rowptr[1] == 0 and np.array_equal(np.diff(g.e_rowptr[1:]), np.ones(g.n - 1))
                and np.array_equal(g.e_col, np.arange(g.n - 1)) and bool((g.e_val != 0).all()))
    def classes(g):
        m = g.sites.reshape(g.n, g.dim).astype(np.float32)
        nz = (m != 0).sum(1)
        return bool((((nz == 1) & (m.max(1) == 1.0)) | (m == np.float32(1.0 / g.dim)).all(1) | (nz == 0)).all())
    return chain(job.g1) and chain(job.g2) and classes(job.g1) and classes(job.g2)


def _table_mode(ctx, b, i):
    """Whether job i of a batch in the product's form took its scores from the class table (then it wrote no S to read back)."""
    import prographmsa_amd as pg
    j = b.cj.jobs[i]
    S = np.zeros(j.g1.n * j.g2.n, np.float32)
    rc = pg.lib.pgm_align_batch_read_matrices(ctx.handle, b.handle, i, None, None, None, None, P(S, C.c_float))
    assert rc in (pg.PGM_OK, pg.PGM_ERR_INVALID)
    return rc == pg.PGM_ERR_INVALID


def _kept_and_product(ctx, js):
    """Every job's M, X, Y, W, S, score and mappings against the oracle (PGM_BATCH_KEEP_MATRICES), then the product's form of
    the same batch (chain-only jobs keep decision bits, jobs of two sequence graphs look their scores up): the same results."""
    from prographmsa_amd import jobs as J
    b = J.Batch(ctx, js, keep_matrices=True)
    b.run()
    res = b.fetch()
    for i, j in enumerate(js):
        _cmp_job(b, i, j, res[i])
    b.close()
    b = J.Batch(ctx, js)
    b.run()
    res2 = b.fetch()
    for i, j in enumerate(js):
        assert _table_mode(ctx, b, i) == _sequence_pair(j), i
    b.close()
    for r, r2 in zip(res, res2):
        _same(r2, r)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("family", sorted(SWEEP_FAMILIES) + ["crit"])
def test_align_graphs_every_dim_bit_exact(ctx, family, dim):
    _kept_and_product(ctx, _jobs(ctx, "dims %s D%d" % (family, dim), A.dims_recipe(family, dim), *A.DIMS_CLAIMS[family]))


@pytest.mark.parametrize("dim", [4, 64])
@pytest.mark.parametrize("case", A.NEW_CASES + ["refusals"])
def test_unreached_paths_smallest_and_largest_dim_bit_exact(ctx, case, dim):
    """test_gpu_align.py's cases for the paths no random_graph job takes (generic nodes of self-contained sweeps, wide workers, kill
    nodes, edges of infinite cost, two edges from one predecessor, the refusals of a MODE 2 sweep) at 4 and 64 states."""
    recipe, claims, named = A.refusal_case(dim) if case == "refusals" else A.new_recipes(dim)[case]
    _kept_and_product(ctx, _jobs(ctx, "%s D%d" % (case, dim), recipe, claims, named))


@pytest.mark.parametrize("dim", DIMS + [20, 61])
def test_sequence_graph_jobs_every_dim(ctx, dim):
    """Batches of several jobs of two sequence graphs (one-hot, uniform 1 / D and empty columns: the lean kernel's class table of
    (D + 2)^2 scores, a header of 2 (D + 2) + 1 ints per job) at lengths with two rows per lane (rshift 1) and several bands; one job
    with a column of no class among them (its scores come from the emission kernel), and the same jobs beside a job with skip
    edges: scores and mappings against the oracle."""
    from prographmsa_amd import jobs as J
    import oracle_lib
    lens = [(1100, 700), (2500, 90), (150, 170), (1, 1), (61, 200), (300, 280)]
    seq = [J.sequence_job(32000 + 100 * dim + k, L1, L2, dim, unknown_frac=0.05 * (k % 3)) for k, (L1, L2) in enumerate(lens)]
    odd = J.sequence_job(32090 + 100 * dim, 120, 140, dim)
    s = odd.g2.sites.reshape(142, dim)
    s[7] = 0.5 / dim                                   # a column that is neither one-hot, nor uniform 1 / D, nor empty
    odd.g2.sites = s.reshape(-1)
    other = J.random_job(32095 + 100 * dim, 260, 240, dim=dim, skip_frac=0.2)
    refs = {}
    for js in (seq, seq[:3] + [odd] + seq[3:], [other] + seq):
        b = J.Batch(ctx, js)
        b.run()
        res = b.fetch()
        for i, j in enumerate(js):   # (a class header that ran into the next job's would take that job out of table mode)
            assert _table_mode(ctx, b, i) == (j is not odd and j is not other), i
        b.close()
        for i, j in enumerate(js):
            if id(j) not in refs:
                refs[id(j)] = oracle_lib.align_graphs(j)
            _same(res[i], refs[id(j)])


@pytest.mark.parametrize("dims", [(4, 20, 21, 61, 64), (1, 4, 19, 20)])
def test_mixed_dim_batches_bit_exact(ctx, dims):
    """Jobs of different alphabet sizes in one batch: the prep and emission kernels are instantiated for the batch's largest
    size, so every job's converted profiles must have the batch's padded stride.  Jobs with skip edges, chain-only jobs with
    random profiles and jobs of two sequence graphs of every size, the sizes interleaved."""
    from prographmsa_amd import jobs as J
    js = []
    for k in range(3):
        for d in dims:
            seed = 33000 + 100 * d + 10 * k
            if k == 0:
                js.append(J.random_job(seed, 260 + 3 * d, 240 - d, dim=d, skip_frac=0.2))
            elif k == 1:
                js.append(J.random_job(seed, 300, 280 + d, dim=d, skip_frac=0.0, drop_chain_frac=0.0))
            else:
                js.append(J.sequence_job(seed, 160 + d, 140, d))
    js.append(J.random_job(33999, 700, 650, dim=dims[-1], skip_frac=0.1, skip_span=70, repeat_frac=0.03, repeat_span=90))
    _kept_and_product(ctx, js)


def test_sizes_outside_the_range_are_rejected(ctx):
    """PGM_ERR_INVALID just outside every entry point's range of alphabet sizes, and a context that still computes afterwards."""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    import oracle_lib
    INV = pg.PGM_ERR_INVALID
    # alignGraphs: 1..64 (per job; a batch with one bad job is refused as a whole)
    good = J.random_job(34000, 30, 28, dim=4, skip_frac=0.2)
    for D in (0, 65):
        cj = J.CJobs([good, J.random_job(34001 + D, 30, 28, dim=max(D, 4), skip_frac=0.2)])
        if D == 0:
            cj._g1[1].dim = cj._g2[1].dim = 0       # (graphs of 4 states that claim none)
        assert pg.lib.pgm_align_graphs_batch(ctx.handle, cj.n, cj.g1, cj.g2, cj.m, cj.sc, cj.out) == INV
        assert b"job 1" in pg.lib.pgm_last_error()
        h = C.c_void_p()
        assert pg.lib.pgm_align_batch_create_ex(ctx.handle, cj.n, cj.g1, cj.g2, cj.m, cj.sc, 0, C.byref(h)) == INV and not h.value
    # merge of profiles and one-hot leaves: 1..64
    for D in (0, 65):
        Dm = max(D, 1)
        g = np.asfortranarray(np.zeros((Dm, 3)))
        Pm = np.asfortranarray(np.eye(Dm))
        k1 = np.arange(3, dtype=np.uint32); fl = np.zeros(3, np.uint8); out = np.zeros(Dm * 3)
        j = pg.pgm_merge_job()
        j.dim, j.n1, j.n2, j.nnodes = D, 3, 3, 3
        j.sites1, j.sites2, j.P1, j.P2 = P(g, C.c_double), P(g, C.c_double), P(Pm, C.c_double), P(Pm, C.c_double)
        j.k1, j.k2, j.g2_with_P1, j.profiles = P(k1, C.c_uint32), P(k1, C.c_uint32), P(fl, C.c_uint8), P(out, C.c_double)
        assert pg.lib.pgm_merge_profiles_batch(ctx.handle, 1, C.byref(j)) == INV
        syms = np.zeros(5, np.int8); offs = np.array([0, 5], np.uint32)
        dev = (C.POINTER(C.c_double) * 1)()
        assert pg.lib.pgm_resident_onehot(ctx.handle, D, 1, P(syms, C.c_int8), P(offs, C.c_uint32), dev) == INV
    # all-pairs NW: 1..61
    syms = np.zeros(10, np.int8); offs = np.array([0, 4, 10], np.uint32)
    pi = np.array([0], np.uint32); pj = np.array([1], np.uint32)
    for D in (0, 62):
        score = np.ones((D + 1) * (D + 1), np.int32)
        counts = np.zeros(max(1, D * D), np.int32); gaps = np.zeros(1, np.uint32)
        assert pg.lib.pgm_nw_pairs_batch(ctx.handle, D, P(score, C.c_int32), -10, -2, 2, P(syms, C.c_int8), P(offs, C.c_uint32), 1,
                                         P(pi, C.c_uint32), P(pj, C.c_uint32), P(counts, C.c_int32), P(gaps, C.c_uint32)) == INV
    # pair counts of an alignment: 20..64
    rows = np.zeros((2, 8), np.int8)
    for D in (19, 65):
        counts = np.zeros(D * D, np.int32); gaps = np.zeros(1, np.uint32)
        assert pg.lib.pgm_prealigned_counts_batch(ctx.handle, D, 2, 8, P(rows, C.c_int8), 1, P(pi, C.c_uint32), P(pj, C.c_uint32),
                                                  P(counts, C.c_int32), P(gaps, C.c_uint32)) == INV
    # ML distances: 1..20
    D = 21
    keep = [np.asfortranarray(np.eye(D)) for _ in range(3)] + [np.zeros(D)]
    m = pg.pgm_mldist_model()
    m.dim = D
    m.Q, m.V, m.Vi, m.sigma = P(keep[0], C.c_double), P(keep[1], C.c_double), P(keep[2], C.c_double), P(keep[3], C.c_double)
    cnt = np.zeros(D * D, np.int32); gaps = np.zeros(1, np.uint32); sl = np.ones(1); dist = np.zeros(1); var = np.zeros(1)
    assert pg.lib.pgm_mldist_batch(ctx.handle, C.byref(m), 1, P(cnt, C.c_int32), P(gaps, C.c_uint32), P(sl, C.c_double),
                                   P(dist, C.c_double), P(var, C.c_double)) == INV
    # the context still computes: alignGraphs at 4 and 64 states, NW pairs at 61
    js = [good, J.random_job(34003, 40, 50, dim=64, skip_frac=0.2)]
    for j, r in zip(js, J.align_graphs_batch(ctx, js)):
        _same(r, oracle_lib.align_graphs(j))
    score = np.ascontiguousarray(np.eye(62, dtype=np.int32).reshape(-1) * 5 - 1)
    syms = np.array([1, 2, 3, 61, 60, 5, 2, 3, 4, 61], np.int8)
    counts = np.zeros(61 * 61, np.int32); gaps = np.zeros(1, np.uint32)
    pg.check(pg.lib.pgm_nw_pairs_batch(ctx.handle, 61, P(score, C.c_int32), -10, -2, 2, P(syms, C.c_int8), P(offs, C.c_uint32), 1,
                                       P(pi, C.c_uint32), P(pj, C.c_uint32), P(counts, C.c_int32), P(gaps, C.c_uint32)))
    co, go_ = oracle_lib.nw_pairs(61, score, -10, -2, syms, offs, pi, pj)
    assert np.array_equal(counts.reshape(1, -1), co) and np.array_equal(gaps, go_)
