"""GPU parity: HIP alignGraphs through the C ABI vs the CPU oracle (bit-exact DP matrices and mappings)."""
import numpy as np
import pytest

import align_cases as A
from align_cases import FAMILIES   # (test_gpu_dims.py takes them from here)

pytestmark = pytest.mark.gpu


def _jobs(ctx, name, recipe, claims=(), named=None):
    """The jobs of a case of align_cases.py, held to what the case claims by the plan of this batch at the device's CU count: on a
    device where the plan sends them elsewhere the test fails with the label's name instead of testing another kernel."""
    js = A.build(recipe)
    A.check_claims(name, js, list(claims), named or {}, ctx.device_info()[1])
    return js


def _cmp_job(batch, idx, job, res):
    import oracle_lib
    assert A.end_is_reachable(job.g1) and A.end_is_reachable(job.g2)   # (the oracle is undefined on a job without an alignment)
    ref = oracle_lib.align_graphs(job, want_matrices=True)
    mats = batch.read_matrices(idx)
    n1, n2 = job.g1.n, job.g2.n
    names = "MXYWS"
    for k in range(5):
        a = mats[k][: n1 - 1, : n2 - 1]
        b = ref["mats"][k][: n1 - 1, : n2 - 1]
        if k == 4:   # S: border row/column 0 hold 0/0 garbage on both sides, never read
            a, b = a[1:, 1:], b[1:, 1:]
        same = (a.view(np.uint32) == b.view(np.uint32))
        assert same.all(), "matrix %s differs at %s (job %d, %dx%d): %r vs %r" % (
            names[k], np.argwhere(~same)[:3], idx, n1, n2, a[~same][:3], b[~same][:3])
    assert res["status"] == ref["status"] == 0
    assert np.float32(res["score"]).view(np.uint32) == np.float32(ref["score"]).view(np.uint32)
    assert res["n_tr_indels"] == ref["n_tr_indels"]
    assert np.array_equal(res["map1"], ref["map1"]) and np.array_equal(res["map2"], ref["map2"])


@pytest.mark.parametrize("dim", [20, 61])
@pytest.mark.parametrize("kw", FAMILIES)
def test_random_jobs_bit_exact(ctx, kw, dim):
    from prographmsa_amd import jobs as J
    fi = next(i for i, f in enumerate(FAMILIES) if f is kw)
    js = _jobs(ctx, "family %d D%d" % (fi, dim), A.family_recipe(fi, dim), A.FAMILY_CLAIMS[fi] + A.FAMILY_CLAIMS_AT.get((fi, dim), []))
    b = J.Batch(ctx, js, keep_matrices=True)
    b.run()
    res = b.fetch()
    for i, j in enumerate(js):
        _cmp_job(b, i, j, res[i])
    b.close()
    # the product's form of the batch (no test hook: chain-only jobs keep decision bytes instead of the matrices): same results
    b = J.Batch(ctx, js)
    b.run()
    res2 = b.fetch()
    for r, r2 in zip(res, res2):
        assert r["status"] == r2["status"] == 0 and r["n_tr_indels"] == r2["n_tr_indels"]
        assert np.float32(r["score"]).view(np.uint32) == np.float32(r2["score"]).view(np.uint32)
        assert np.array_equal(r["map1"], r2["map1"]) and np.array_equal(r["map2"], r2["map2"])
    if kw.get("skip_frac", 1) == 0.0 and len(js) > 12:
        import prographmsa_amd as pg
        with pytest.raises(pg.PgmError):
            b.read_matrices(12)   # not kept
    b.close()


def test_large_heavy_tailed_jobs_bit_exact(ctx):
    """Jobs of the size of the roots of configs 3-5 with heavy-tailed edge lengths: dozens of MODE 2 bands with long column
    entries, remote row entries and overflow columns in flight at once (tools/probe_big.py goes to 6000 x 5000).  Every job has nodes
    of the generic path (a column with more than three long entries, or past the overflow table's 128 records: the plan does not say which)."""
    from prographmsa_amd import jobs as J
    js = _jobs(ctx, "large_heavy", A.LARGE_HEAVY, (), A.LARGE_HEAVY_CLAIMS)
    b = J.Batch(ctx, js, keep_matrices=True)
    b.run()
    res = b.fetch()
    for i, j in enumerate(js):
        _cmp_job(b, i, j, res[i])
    b.close()


def test_critical_path_kernel_and_wide_bands_bit_exact(ctx):
    """A batch that does not fill a device of 256 CUs, 20 and 61 states (align_cases.crit_wide_recipe says what the plan makes of every
    job): two MODE 2 jobs with remote row entries, the longer one in the launch of the longest chains; five crit3 jobs of 7 to 21 bands
    that share the main launch with the other one, so that pgm_fill_kernel sweeps them (pgm_crit_kernel sweeps a launch of crit3 jobs
    only: the families 3-7 above, test_job_modes_of_small_and_large_batches, the long job of the wide cases below); and one job of 5 bands
    with a 32-step history on a wide worker of pgm_band_kernel.  All four DP matrices, scores and mappings against the oracle; in one
    batch, so that workers take several bands one after another."""
    from prographmsa_amd import jobs as J
    for dim in (20, 61):
        js = _jobs(ctx, "crit_wide D%d" % dim, A.crit_wide_recipe(dim), *A.CRIT_WIDE_CLAIMS)
        b = J.Batch(ctx, js, keep_matrices=True)
        b.run()
        res = b.fetch()
        for i, j in enumerate(js):
            _cmp_job(b, i, j, res[i])
        b.close()


def test_job_modes_of_small_and_large_batches_bit_exact(ctx):
    """Four probes of 5 to 15 bands alone, among 22 fillers of 2000 x 2000 and among 64 fillers of 900 x 900 (at 256 CUs; asserted from
    the plan, here and in test_cpu_align_reach.py).  Alone the batch does not fill the device and every job of 8 bands or more is promoted
    to MODE 2 (pgm_align_batch_create: a guide-tree level on its own): probe 0, with remote row entries, is the launch of the longest
    chains on pgm_fill_kernel, probes 1-3 are crit3 jobs and the main launch is pgm_crit_kernel's.  Among the big fillers nothing is
    promoted and the longest chain is long: probe 3 becomes a self-contained sweep on a wide worker of pgm_band_kernel, probes 1 and 2
    stay crit3 jobs (their histories do not fit a wide worker's slot) but share the main launch with probe 0, so pgm_fill_kernel sweeps
    them, and the fillers are pgm_crit_kernel's.  Among the 64 fillers of old every probe keeps the kernel it has alone — what differs
    is the order of the lists and the workers — and the fillers, in one launch with probe 0, are swept by pgm_fill_kernel.
    Every way: all four DP matrices, scores and mappings of the probes against the oracle, and the mappings of every ninth filler."""
    from prographmsa_amd import jobs as J
    import oracle_lib
    probes = A.PROBES
    for name, fill in (("alone", []), ("big fillers", A.BIG_FILLERS), ("fillers", A.FILLERS)):
        js = _jobs(ctx, "modes " + name, probes + fill, *A.MODES_CLAIMS[name])
        b = J.Batch(ctx, js, keep_matrices=True)
        b.run()
        res = b.fetch()
        for i in range(len(probes)):
            _cmp_job(b, i, js[i], res[i])
        for i in range(len(probes), len(js), 9):
            ref = oracle_lib.align_graphs(js[i])
            assert res[i]["status"] == 0 and np.array_equal(res[i]["map1"], ref["map1"]) and np.array_equal(res[i]["map2"], ref["map2"]), i
        b.close()


def test_handoff_timeout_in_the_critical_path_kernel(ctx):
    """The same time-out path as below for a job swept by pgm_crit_kernel: band 3 never publishes its progress, the chain wavefront of band 4
    gives up, raises the abort flag, every wavefront of every worker leaves, the batch reports PGM_ERR_DEVICE — and runs clean afterwards."""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    import oracle_lib
    js = [J.random_job(7600, 1400, 600, skip_frac=0.2, skip_span=20, skip_max=2, drop_chain_frac=0.0)]
    b = J.Batch(ctx, js)
    pg.check(pg.lib.pgm_align_batch_test_stall(b.handle, 0, 3, 2000))
    b.run()
    rc = pg.lib.pgm_align_batch_fetch(ctx.handle, b.handle, b.cj.out)
    assert rc == pg.PGM_ERR_DEVICE and b"timed out" in pg.lib.pgm_last_error()
    pg.check(pg.lib.pgm_align_batch_test_stall(b.handle, 0xFFFFFFFF, 0, 0))
    b.run()
    res = b.fetch()
    ref = oracle_lib.align_graphs(js[0])
    assert res[0]["status"] == 0 and np.array_equal(res[0]["map1"], ref["map1"]) and np.array_equal(res[0]["map2"], ref["map2"])
    b.close()


def test_relaunch_and_fetch(ctx):
    """run, run, fetch and run, fetch, fetch: the result records in the pinned block are reset by every launch and copied
    out by fetch while the kernel is still running (status word last); every fetch returns the same results."""
    from prographmsa_amd import jobs as J
    js = [J.random_job(300 + i, 260 + 37 * i, 300 - 11 * i, skip_frac=0.2) for i in range(12)]
    b = J.Batch(ctx, js, keep_matrices=True)
    b.run(); b.run()
    r1 = b.fetch()
    b.run()
    r2 = b.fetch()
    r3 = b.fetch()
    for a in (r2, r3):
        for x, y in zip(r1, a):
            assert np.array_equal(x["map1"], y["map1"]) and np.array_equal(x["map2"], y["map2"])
            assert np.float32(x["score"]).view(np.uint32) == np.float32(y["score"]).view(np.uint32) and x["status"] == y["status"] == 0
    for i, j in enumerate(js):
        _cmp_job(b, i, j, r1[i])
    b.close()


def test_one_call_entry_point(ctx):
    import oracle_lib
    from prographmsa_amd import jobs as J
    js = [J.random_job(7 + i, 90 + 13 * i, 120 - 7 * i, skip_frac=0.15) for i in range(5)]
    res = J.align_graphs_batch(ctx, js)
    for j, r in zip(js, res):
        ref = oracle_lib.align_graphs(j)
        assert np.array_equal(r["map1"], ref["map1"]) and np.array_equal(r["map2"], ref["map2"])
        assert np.float32(r["score"]).view(np.uint32) == np.float32(ref["score"]).view(np.uint32)


def test_invalid_graphs_are_rejected(ctx):
    """PGM_ERR_INVALID: an edge to a later node (Graph.h:43 guarantees from < to) and a dimension mismatch."""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    good = J.random_job(5, 30, 28, skip_frac=0.2)
    bad = J.random_job(6, 30, 28, skip_frac=0.2)
    bad.g1.e_col[int(bad.g1.e_rowptr[10])] = 17          # node 10 <- node 17
    cj = J.CJobs([good, bad])
    rc = pg.lib.pgm_align_graphs_batch(ctx.handle, cj.n, cj.g1, cj.g2, cj.m, cj.sc, cj.out)
    assert rc == pg.PGM_ERR_INVALID and b"job 1" in pg.lib.pgm_last_error()
    mism = J.random_job(7, 30, 28, skip_frac=0.2)
    other = J.random_job(8, 30, 28, dim=61, skip_frac=0.2)
    mism.g2 = other.g2                                    # 20-state graph against a 61-state graph
    cj = J.CJobs([mism])
    rc = pg.lib.pgm_align_graphs_batch(ctx.handle, cj.n, cj.g1, cj.g2, cj.m, cj.sc, cj.out)
    assert rc == pg.PGM_ERR_INVALID
    # the context is still usable afterwards
    assert J.align_graphs_batch(ctx, [good])[0]["status"] == 0


def test_handoff_timeout_aborts_the_batch(ctx):
    """PGM_ERR_DEVICE: band 0 of job 0 never publishes its progress (test knob), the band below times out after a
    shortened spin limit, raises the abort flag and every job of the batch reports a device error instead of hanging."""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    js = [J.random_job(21, 200, 150, skip_frac=0.2), J.random_job(22, 90, 80, skip_frac=0.0, drop_chain_frac=0.0)]
    b = J.Batch(ctx, js)
    pg.check(pg.lib.pgm_align_batch_test_stall(b.handle, 0, 0, 2000))
    b.run()
    rc = pg.lib.pgm_align_batch_fetch(ctx.handle, b.handle, b.cj.out)
    assert rc == pg.PGM_ERR_DEVICE and b"timed out" in pg.lib.pgm_last_error()
    pg.check(pg.lib.pgm_align_batch_test_stall(b.handle, 0xFFFFFFFF, 0, 0))
    b.run()                                               # the same batch runs clean afterwards
    res = b.fetch()
    import oracle_lib
    for j, r in zip(js, res):
        ref = oracle_lib.align_graphs(j)
        assert r["status"] == 0 and np.array_equal(r["map1"], ref["map1"]) and np.array_equal(r["map2"], ref["map2"])
    b.close()


def test_job_timeline(ctx):
    """pgm_align_batch_job_times: every job of a mixed batch (chain-only jobs in the lean kernel, bands one per wavefront, a MODE 2 job
    with a pre-linked corridor) has a sweep end and a later publication stamp, all within the launch; pgm_align_batch_stage_times
    counts exactly the fetched launches."""
    import ctypes as C
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    js = [J.random_job(900 + i, n1, n2, **kw) for i, (n1, n2, kw) in enumerate([
        (300, 280, dict(skip_frac=0.0, drop_chain_frac=0.0)), (500, 510, dict(skip_frac=0.2)), (260, 300, dict(skip_frac=0.3, repeat_frac=0.05)),
        (1400, 1350, dict(skip_frac=0.25, skip_span=27, skip_max=2)), (90, 80, dict(skip_frac=0.0, drop_chain_frac=0.0))])]
    b = J.Batch(ctx, js)
    for _ in range(3):
        b.run(); res = b.fetch()
    assert all(r["status"] == 0 for r in res)
    t = np.zeros(2 * len(js), np.uint64)
    pg.check(pg.lib.pgm_align_batch_job_times(ctx.handle, b.handle, t.ctypes.data_as(C.POINTER(C.c_uint64))))
    t = t.reshape(-1, 2).astype(np.int64)
    assert (t > 0).all() and (t[:, 1] >= t[:, 0]).all()
    assert (t.max() - t.min()) < 100 * 100000          # within 100 ms (10 ns ticks)
    ms = b.stage_times(reset=True)
    assert ms[3] == 3 and ms[2] > 0 and b.stage_times()[3] == 0
    import oracle_lib
    for j, r in zip(js, res):
        ref = oracle_lib.align_graphs(j)
        assert np.array_equal(r["map1"], ref["map1"]) and np.array_equal(r["map2"], ref["map2"])
    b.close()


def test_empty_batch(ctx):
    from prographmsa_amd import jobs as J
    assert J.align_graphs_batch(ctx, []) == []


def test_sequence_graph_jobs_score_table_after_other_batches(ctx):
    """Chain-only jobs of two SEQUENCE graphs (every profile column one-hot, uniform or empty) take their scores from a per-job class
    table instead of the score matrix, and pgm_prep_kernel only works on the slices that hold a class's representative node or the END
    node (PgmJob::cls1, pgm_classify_kernel, pgm_lean_kernel).  Batches of such jobs on a context whose cached buffers earlier batches
    of other shapes have used (round 4: the END node's edge record of a skipped slice was read stale — found by tools/fuzz_e2e.py on
    the second pass of a run), 20 and 61 states, residues without a value: scores and mappings against the oracle."""
    from prographmsa_amd import jobs as J
    import oracle_lib
    seqjob = J.sequence_job   # (5 % residues without a value)
    for D in (20, 61):
        for rnd in range(3):
            mixed = [J.random_job(9100 + 10 * rnd + k, 300 + 37 * k, 280 + 41 * k, dim=D, skip_frac=0.2) for k in range(3)] + \
                    [seqjob(9200 + 10 * rnd + k, 150 + 61 * k, 170 + 53 * k, D) for k in range(3)]
            only = [seqjob(9300 + 10 * rnd + k, 120 + 47 * k + 13 * rnd, 140 + 43 * k + 7 * rnd, D) for k in range(6)]
            for js in (mixed, only):
                b = J.Batch(ctx, js); b.run(); res = b.fetch(); b.close()
                for i, j in enumerate(js):
                    ref = oracle_lib.align_graphs(j)
                    assert np.float32(res[i]["score"]).view(np.uint32) == np.float32(ref["score"]).view(np.uint32), (D, rnd, i)
                    assert np.array_equal(res[i]["map1"], ref["map1"]) and np.array_equal(res[i]["map2"], ref["map2"]), (D, rnd, i)


@pytest.mark.parametrize("dim", [20, 61])
@pytest.mark.parametrize("case", A.NEW_CASES)
def test_unreached_paths_bit_exact(ctx, case, dim):
    """The paths no random_graph job takes (align_cases.new_recipes: generic nodes of self-contained sweeps, more than one wide job, kill
    nodes, edges of infinite cost, a broken chain, two edges from one predecessor): M, X, Y, W, S, score and mappings of every job
    against the oracle, with the matrices kept and in the product's form."""
    from test_gpu_dims import _kept_and_product
    recipe, claims, named = A.new_recipes(dim)[case]
    _kept_and_product(ctx, _jobs(ctx, "%s D%d" % (case, dim), recipe, claims, named))


@pytest.mark.parametrize("dim", [20, 61])
def test_mode2_refusals_bit_exact(ctx, dim):
    """Each rule by which a node of a MODE 2 job goes to the generic path (align_cases.refusal_recipes), the hub one entry past the limit
    and, in the control, at it: every job against the oracle."""
    from test_gpu_dims import _kept_and_product
    recipe, claims, named = A.refusal_case(dim)
    js = _jobs(ctx, "refusals D%d" % dim, recipe, claims, named)
    gen = A.generic_nodes(js, ctx.device_info()[1])
    assert all(gen[k] > gen[k + 1] for k in range(0, len(js), 2)), gen
    _kept_and_product(ctx, js)
