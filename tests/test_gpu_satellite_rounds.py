"""The satellite kernels on the MI355X past their staging pieces and launch caps: every case of tests/test_cpu_satellite_rounds.py (which
holds the lists, derives each size from the cap in the kernel header or the launch code, and says what each case is for) against the
statements the kernels' own files use, bit for bit or as exact integers, every output preset to garbage by the helpers of those files.

1. BioNJ by the criterion at PGM_BIONJ_CHUNK + 16 taxa (the chunk loops' second lap), solo and in one pgm_bionj_multi call; 65539
   families in one call of pgm_bionj_multi and of pgm_bionj_plan_multi (blockIdx.z).  The third chunk (2049 taxa and more) is
   deliberately left out: the numpy statement takes about a minute there, and the chunk loops are generic in k0.
2. pgm_transfer_min and pgm_transfer_taxa at 513 to 2049 leaves (one, two and three slabs of PGM_TRANSFER_K words) and at 65537 replicates.
3. pgm_wls_pair_sums_batch at 66 blocks of PGM_WLS_ROWS rows and at more jobs than the 64 MB of block partials hold.
4. pgm_gap_parsimony_batch at more than 256 blocks per candidate and at more candidates than the 256 MB of scratch hold;
   pgm_gapmask_extend_batch at 65540 jobs.
5. pgm_prealigned_counts_resampled at more pairs than one round of the grid and at 65537 replicates.
6. One driver run of 1040 taxa on the default route against the oracle driver.

Whoever moves one of those caps moves the case with it: the sizes are computed from the cap (the test notes of 3.8, 3.9, 3.11,
3.13, 3.15 and 3.16)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import batch_util as bu
import bionj_ref as B
import gen
import test_cpu_satellite_rounds as SR
import test_gpu_bionj as TB
import test_gpu_bootstrap as TS
import test_gpu_reroot as TR
import test_gpu_taxa as TT
import test_gpu_transfer as TG
import test_gpu_wls as TW

pytestmark = pytest.mark.gpu
GARBAGE = TG.GARBAGE


# ---- 1: BioNJ ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SR.BIONJ_KINDS)
def test_bionj_second_lap_of_the_chunk_loops(ctx, kind):
    """1040 taxa: the joins 0..15 have dim 1040..1025 > PGM_BIONJ_CHUNK, so pgm_bionj_sums_kernel's loop over k0 takes a second lap at
    step 0 (the clamping branch) and at steps > 0 (the gather through act): the re-alignment of the four accumulators at k < k0, the odd
    last pair and the tail in the second chunk, every residue of dim mod 4 and both parities of start; pgm_bionj_join_kernel's vsum loop
    takes its second lap in the same joins (at least 8 of them with 0 < lambda < 1: tests/test_cpu_satellite_rounds.py)."""
    n = SR.BIONJ_N
    assert n - (SR.BIONJ_PAST - 1) > SR.BIONJ_CHUNK
    D, V, ref_j, ref_f, info = SR.bionj_case(kind)
    D0, V0 = D.copy(), V.copy()
    got_j, got_f, launches = TB.device_solo(ctx, D, V)
    assert B.same_bits(D, D0) and B.same_bits(V, V0)   # the inputs are not modified
    TB.assert_record(got_j, got_f, ref_j, ref_f, "%s n = %d" % (kind, n))
    assert launches > 0 and launches % (n - 3) == 0


def test_bionj_multi_with_two_families_past_the_chunk(ctx):
    """One pgm_bionj_multi call over (asym, 1040), (ties, 5), (lambda, 1040), (random, 130): the second lap of the chunk loops with
    the families on blockIdx.y, two of them done long before the others.  Every family equals its solo call and the statement, and the
    call launches what the solo call at 1040 taxa launches."""
    mats = [TB.case(k, n)[:2] for k, n in SR.BIONJ_MULTI]
    assert max(n for _, n in SR.BIONJ_MULTI) - (SR.BIONJ_PAST - 1) > SR.BIONJ_CHUNK
    mj, mf, launches = TB.device_multi(ctx, mats)
    solo_launches = {}
    for (D, V), (k, n), gj, gf in zip(mats, SR.BIONJ_MULTI, mj, mf):
        sj, sf, solo_launches[n] = TB.device_solo(ctx, D, V)
        assert B.same_bits(gj, sj) and B.same_bits(gf, sf), (k, n)
        TB.assert_record(gj, gf, TB.case(k, n)[2], TB.case(k, n)[3], "multi %s n = %d" % (k, n))
    assert launches == solo_launches[SR.BIONJ_N]


def _many_families(ctx, plan):
    """BIONJ_FAMILIES small families in one call (by the plans of tests/topology_ref.py if `plan`), family f the matrices number f % 7;
    every join record and every final_d against the seven statements tiled."""
    import prographmsa_amd as pg
    nfam = SR.BIONJ_FAMILIES
    assert nfam > SR.GRID_Y   # gz = 2
    crit, planned = SR.bionj_small()
    fams = planned if plan else crit
    ns = np.ascontiguousarray(np.tile(np.array(SR.BIONJ_SMALL_NS, np.uint32), nfam // 7 + 1)[:nfam])
    Dcat, Vcat = SR.tiled_families([f[0] for f in fams], nfam), SR.tiled_families([f[1] for f in fams], nfam)
    want_j, want_f = SR.tiled_families([f[-2] for f in fams], nfam), SR.tiled_families([f[-1] for f in fams], nfam)
    assert len(want_j) == int((ns.astype(np.int64) - 3).sum()) and len(want_f) == 9 * nfam and len(Dcat) == int((ns.astype(np.int64) ** 2).sum())
    joins = np.zeros(len(want_j) + 1, B.JOIN_DTYPE)
    joins.view(np.uint8)[:] = 0xA5
    final_d = np.full(9 * nfam, -1.0)
    PN, PJ = ns.ctypes.data_as(C.POINTER(C.c_uint32)), joins.ctypes.data_as(C.POINTER(pg.pgm_bionj_join))
    if plan:
        pairs = SR.tiled_families([np.array(f[2][:n - 3], np.uint32).reshape(-1, 2) for f, n in zip(fams, SR.BIONJ_SMALL_NS)], nfam)
        assert len(pairs) == 2 * len(want_j)
        rc = pg.lib.pgm_bionj_plan_multi(ctx.handle, nfam, PN, TB.PD(Dcat), TB.PD(Vcat), pairs.ctypes.data_as(C.POINTER(pg.pgm_bionj_pair)), PJ, TB.PD(final_d))
    else:
        rc = pg.lib.pgm_bionj_multi(ctx.handle, nfam, PN, TB.PD(Dcat), TB.PD(Vcat), PJ, TB.PD(final_d))
    assert rc == 0, (rc, pg.lib.pgm_last_error())
    joff = np.concatenate([[0], np.cumsum(ns.astype(np.int64) - 3)])
    bad_j = np.flatnonzero((joins[:-1].view(np.uint8).reshape(-1, B.JOIN_DTYPE.itemsize) != want_j.view(np.uint8).reshape(-1, B.JOIN_DTYPE.itemsize)).any(axis=1))
    assert bad_j.size == 0, "join records of %d families differ, first family %d" % (len(set(np.searchsorted(joff, bad_j, "right") - 1)), np.searchsorted(joff, bad_j[0], "right") - 1)
    bad_f = np.flatnonzero((final_d.view(np.uint64) != want_f.view(np.uint64)).reshape(nfam, 9).any(axis=1))
    assert bad_f.size == 0, "final_d of %d families differs, first family %d" % (bad_f.size, bad_f[0])
    assert joins[-1:].view(np.uint8).min() == 0xA5   # (nothing past the last record)
    return pg.lib.pgm_bionj_last_launches(ctx.handle)


def test_bionj_multi_more_families_than_grid_y(ctx):
    """65539 families of 4 to 6 taxa in one pgm_bionj_multi call: gy = 65535 and gz = 2, so the families 65535.. come from the
    blockIdx.z half of pgm_bionj_family() in the sums, scan and join kernels.  Every family is checked."""
    assert _many_families(ctx, plan=False) == 3 * (max(SR.BIONJ_SMALL_NS) - 3)


def test_bionj_plan_multi_more_families_than_grid_y(ctx):
    """The same 65539 families through pgm_bionj_plan_multi: the blockIdx.z half of pgm_bionj_family() in pgm_bionj_prepare_kernel and
    pgm_bionj_plan_kernel."""
    assert 0 < _many_families(ctx, plan=True) <= 3


# ---- 2: transfer bootstrap, taxon instability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nleaves", SR.TRANSFER_LEAVES)
def test_transfer_min_past_one_slab_of_words(ctx, nleaves):
    """pgm_transfer_min_kernel<false>: 513 leaves are 18 words, the second lap of the clamp's popcount loop over 16 threads; 1023 and
    1024 leaves one full slab of PGM_TRANSFER_K words; 1025 a second lap of the loop over w0 with two words in it; 2049 a third.  The
    first 40 sets of replicate 0 differ from reference set k in leaves of the later slabs only, so dropping a slab gives 0 for 1 or 7."""
    case = SR.transfer_case(nleaves)
    words32 = 2 * ((nleaves + 63) // 64)
    assert (words32 > SR.TRANSFER_K) == (nleaves > SR.SLAB)
    phi = TG.device_phi(ctx, nleaves, case["ref"], case["reps"])
    want = np.array(case["phi"], np.uint32)
    assert np.array_equal(phi, want), np.argwhere(phi != want)[:5].tolist()


@pytest.mark.parametrize("nleaves", SR.TRANSFER_LEAVES)
def test_transfer_taxa_past_one_slab_of_words(ctx, nleaves):
    """pgm_transfer_min_kernel<true> over the same laps of w0 (the keys carry arg and flip), and pgm_transfer_moved_kernel over 3, 4, 5
    and 9 tiles of 256 leaves: phi, arg, moved and counted; the threshold counts the 40 near sets, and the moved leaves are exactly the
    leaves of the later slabs they were flipped in."""
    case = SR.transfer_case(nleaves)
    got = TT.device_taxa(ctx, nleaves, case["ref"], case["thr"], case["reps"])
    for name, g, w in zip(("phi", "arg", "moved", "counted"), got, case["taxa"]):
        w = np.array(w, np.uint32).reshape(g.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())
    phi, arg, moved, counted = got
    for k in range(SR.TRANSFER_NEAR):
        assert np.flatnonzero(moved[k]).tolist() == case["flipped"][k]
    assert counted.sum() == SR.TRANSFER_NEAR and moved[SR.TRANSFER_NEAR:].sum() == 0


def test_transfer_more_replicates_than_grid_y(ctx):
    """65537 replicates of 0, 1 and 2 sets over five leaves: the launches of both entries have 65535 workgroups along blockIdx.y, and the
    loop `r += gridDim.y` of pgm_transfer_min_kernel takes a second replicate in two of them (<false> and <true>);
    pgm_transfer_moved_kernel stages 257 chunks of 256 replicates.  Every column of phi is checked, and arg, moved and counted."""
    case = SR.transfer_reps_case()
    n = SR.TRANSFER_REPS_LEAVES
    assert len(case["reps"]) == SR.TRANSFER_REPS > SR.GRID_Y
    want = np.array(case["phi"], np.uint32)
    phi = TG.device_phi(ctx, n, case["ref"], case["reps"])
    assert np.array_equal(phi, want), np.argwhere(phi != want)[:5].tolist()
    got = TT.device_taxa(ctx, n, case["ref"], case["thr"], case["reps"])
    for name, g, w in zip(("phi", "arg", "moved", "counted"), got, case["taxa"]):
        w = np.array(w, np.uint32).reshape(g.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())


# ---- 3: WLS pair sums ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wls_case():
    """(D, W, the five jobs of test_gpu_wls.test_pair_sums_kernel) at WLS_N rows."""
    n = SR.WLS_N
    rng = np.random.default_rng(n)
    D, W = TW.make_matrices(rng, n)
    jobs = [TW.make_job(rng, n, K) + (K,) for K in (4, 5, 4, 5)]
    jobs.append(TW.make_job(rng, n, 5, empty=2) + (5,))
    return D, W, jobs


def test_wls_more_blocks_than_lanes_of_the_jobs_kernel(ctx):
    """1041 rows are 66 blocks of PGM_WLS_ROWS: the loop `b += 64` of pgm_wls_jobs_kernel gives lanes 0 and 1 a second block partial.
    The five jobs against the fsum statement and, bit for bit, the numpy statement of the summation order."""
    import prographmsa_amd as pg
    D, W, jobs = wls_case()
    assert SR.wls_blocks(len(D)) > SR.WLS_LANES
    TW.load(ctx, pg, D, W)
    out = TW.run_kernel(ctx, pg, jobs)
    assert pg.lib.pgm_wls_last_launches(ctx.handle) == 2
    for (lab, off, K), o in zip(jobs, out):
        TW.check_job(o, D, W, lab, off, K, exact=True)
    for i, job in enumerate(jobs):
        assert np.array_equal(TW.run_kernel(ctx, pg, [job])[0], out[i])


def test_wls_more_jobs_than_one_launch_holds(ctx):
    """chunk + 3 jobs on the same matrices, chunk = 64 MB / (66 blocks x 20 slots x 8 bytes): the launch loop of
    pgm_wls_pair_sums_batch runs twice, the second pair of launches reading the job descriptors from j0 on, reusing the block partials
    and writing out from 20 j0 on.  The jobs around the seam exactly, 16 others against a call of their own."""
    import prographmsa_amd as pg
    D, W, _ = wls_case()
    n, chunk = SR.WLS_N, SR.wls_chunk(SR.WLS_N)
    assert SR.WLS_JOBS == chunk + 3 > chunk
    rng = np.random.default_rng(5 * n)
    jobs = [TW.make_job(rng, n, 4 + i % 2) + (4 + i % 2,) for i in range(SR.WLS_JOBS)]
    TW.load(ctx, pg, D, W)
    out = TW.run_kernel(ctx, pg, jobs)
    assert pg.lib.pgm_wls_last_launches(ctx.handle) == 4
    assert not np.isnan(out).any()   # (run_kernel presets NaN)
    for i in (0, chunk - 1, chunk, chunk + 1, chunk + 2):
        TW.check_job(out[i], D, W, *jobs[i], exact=True)
        assert np.array_equal(TW.run_kernel(ctx, pg, [jobs[i]])[0], out[i]), i
    for i in sorted(set(int(i) for i in rng.integers(1, chunk - 1, 16))):
        assert np.array_equal(TW.run_kernel(ctx, pg, [jobs[i]])[0], out[i]), i


# ---- 4: gap parsimony, gap masks ----------------------------------------------------------------------------------------------------------
def _candidate(rng, nl, L):
    return rng.random((nl, L)) < rng.choice([0.05, 0.3, 0.7]), TR.random_topology(rng, nl)


def test_parsimony_more_blocks_than_lanes(ctx):
    """8193, 8225 and 16417 columns are 257, 258 and 514 blocks of 32: the loop `b += blockDim.x` of pgm_gap_parsimony_kernel gives
    lane 0 (lanes 0 and 1) the block l + 256 and, in the last shape, l + 512, and the scratch rows are read back at that stride."""
    import prographmsa_amd as pg
    rng = np.random.default_rng(8193)
    cands = [_candidate(rng, nl, L) for nl, L in SR.PARS_SHAPES]
    assert all(SR.pars_blocks(g.shape[1]) > SR.PARS_LANES for g, _ in cands)
    rc, scores = TR.run_parsimony(ctx, cands)
    pg.check(rc)
    want = [TR.parsimony_np(g, t) for g, t in cands]
    assert [int(s) for s in scores] == want and min(want) > 0


def test_parsimony_more_candidates_than_the_scratch_holds(ctx):
    """One candidate of 1024 rows x 4097 columns needs 1022 x 129 words of consensus scratch, so the 256 MB budget gives 254
    workgroups for the 302 candidates of the call: the loop `j += gridDim.x` of pgm_gap_parsimony_kernel takes a second candidate in
    48 workgroups, and workgroup 0 walks the large candidate and then the one of 64 x 8225 (another block stride) over one scratch
    region.  Every score is checked."""
    import prographmsa_amd as pg
    shapes, at = SR.pars_budget_shapes()
    grid = SR.pars_grid(shapes)
    assert grid == at < len(shapes)
    rng = np.random.default_rng(4097)
    cands = [_candidate(rng, nl, L) for nl, L in shapes]
    rc, scores = TR.run_parsimony(ctx, cands)
    pg.check(rc)
    want = [TR.parsimony_np(g, t) for g, t in cands]
    bad = [k for k in range(len(cands)) if int(scores[k]) != want[k]]
    assert not bad, (bad[:8], [int(scores[k]) for k in bad[:8]], [want[k] for k in bad[:8]])
    assert want[0] > 0 and want[grid] > 0


def test_gapmask_more_jobs_than_the_grid(ctx):
    """65540 jobs of one row, one column extended to two, the gap in front or behind in turn: the loop `j += gridDim.x` of
    pgm_gapmask_extend_kernel takes a second job in five of the 65535 workgroups.  Every output word is checked."""
    import prographmsa_amd as pg
    n = SR.GAPMASK_JOBS
    assert n > SR.GRID_Y
    rng = np.random.default_rng(65540)
    child = (rng.random(n) < 0.5).astype(np.uint64)
    behind = np.arange(n) % 2 == 0                                         # the gap goes behind the child's column, else in front
    src = np.ascontiguousarray(child)
    maps = np.ascontiguousarray(np.where(behind[:, None], [1, pg.PGM_GAP], [pg.PGM_GAP, 1]).astype(np.uint32))
    dst = np.full(n, 0xDEAD, np.uint64)
    rec = np.zeros(n, np.dtype(dict(names=["src", "mapping", "dst", "nrows", "ncols_in", "ncols_out"], formats=["<u8", "<u8", "<u8", "<u4", "<u4", "<u4"],
                                    offsets=[0, 8, 16, 24, 28, 32], itemsize=C.sizeof(pg.pgm_gapmask_job))))
    assert rec.itemsize == 40 and pg.pgm_gapmask_job.nrows.offset == 24 and pg.pgm_gapmask_job.ncols_out.offset == 32
    rec["src"] = src.ctypes.data + 8 * np.arange(n, dtype=np.uint64)
    rec["mapping"] = maps.ctypes.data + 8 * np.arange(n, dtype=np.uint64)
    rec["dst"] = dst.ctypes.data + 8 * np.arange(n, dtype=np.uint64)
    rec["nrows"], rec["ncols_in"], rec["ncols_out"] = 1, 1, 2
    pg.check(pg.lib.pgm_gapmask_extend_batch(ctx.handle, n, rec.ctypes.data_as(C.POINTER(pg.pgm_gapmask_job))))
    want = np.where(behind, child | np.uint64(2), (child << np.uint64(1)) | np.uint64(1))   # a gap column is a 1
    assert np.array_equal(dst, want), np.flatnonzero(dst != want)[:8].tolist()
    for k in (0, 1, n - 2, n - 1):   # (the vectorised expectation is tests/test_gpu_reroot._extend_np's)
        assert dst[k:k + 1].tolist() == TR.pack(TR._extend_np(child[k:k + 1, None].astype(bool), maps[k])).reshape(-1).tolist()


# ---- 5: resampled pair counts -------------------------------------------------------------------------------------------------------------
def _counts_np(dim, rows, cols, pi, pj):
    """The counts and gap openings of pgm_prealigned_counts_resampled in numpy, one step per column (independent of the device)."""
    counts = np.zeros((len(cols), len(pi), dim * dim), np.int32)
    gaps = np.zeros((len(cols), len(pi)), np.uint32)
    for r, c in enumerate(cols):
        a, b = rows[:, c][pi].astype(np.int64), rows[:, c][pj].astype(np.int64)
        last = np.full(len(pi), 3)
        for k in range(a.shape[1]):
            g1, g2 = a[:, k] == -1, b[:, k] == -1
            ty = np.where(~g1 & ~g2, 0, np.where(g1 & g2, 3, np.where(~g1, 1, 2)))
            both = (ty == 0) & (a[:, k] >= 0) & (b[:, k] >= 0)
            np.add.at(counts[r], (np.flatnonzero(both), (a[:, k] + dim * b[:, k])[both]), 1)
            gaps[r] += ((ty == 1) | (ty == 2)) & (ty != last)
            last = np.where(ty != 3, ty, last)
    return counts, gaps


def test_resampled_counts_more_pairs_than_one_round_of_the_grid(ctx):
    """The pairs of 129 rows at 256 CUs (the smallest count above 32 pairs per CU and three more): the launch of
    pgm_prealigned_resampled_kernel has 8 workgroups of four pairs per CU, and the loop `pair += gridDim.x * 4` takes a second pair in
    some wavefronts.  Two replicates, against pgm_prealigned_counts_batch on the gathered matrices and against numpy."""
    import prographmsa_amd as pg
    cus = ctx.device_info()[1]
    n, L, dim = SR.resample_rows(cus), SR.RESAMPLE_L, SR.RESAMPLE_DIM
    pi, pj = TS._all_pairs(n)
    assert len(pi) > SR.RESAMPLE_PAIRS * SR.RESAMPLE_BLOCKS_PER_CU * cus + 3
    rng = np.random.default_rng(129)
    rows = TS._rows(rng, dim, n, L)
    cols = np.array([TS._cols(rng, "random", L), TS._cols(rng, "reversal", L)], np.uint32)
    counts, gaps = ctx.prealigned_counts_resampled(dim, rows, cols, pi, pj)
    rc, rg = TS._reference(pg, ctx, dim, rows, cols, pi, pj)
    assert counts.shape == rc.shape and np.array_equal(counts, rc) and np.array_equal(gaps, rg)
    nc, ng = _counts_np(dim, rows, cols, pi, pj)
    assert np.array_equal(counts, nc) and np.array_equal(gaps, ng)
    assert gaps.max() > 0 and counts.sum() > 0


def test_resampled_counts_more_replicates_than_grid_y(ctx):
    """65537 replicates of two rows and three columns: 65535 workgroups along blockIdx.y, and the loop `rep += gridDim.y` of
    pgm_prealigned_resampled_kernel takes a second replicate in two of them.  Replicate r draws column vector r % 7; the expectation is
    that of the seven, tiled."""
    import prographmsa_amd as pg
    nrep, dim = SR.RESAMPLE_REPS, SR.RESAMPLE_DIM
    assert nrep > SR.GRID_Y
    rows = np.array([[0, 1, -1], [2, 3, 3]], np.int8)
    seven = np.array([[0, 1, 2], [2, 0, 2], [0, 0, 0], [1, 1, 2], [2, 2, 1], [1, 0, 1], [0, 2, 2]], np.uint32)
    pi, pj = TS._all_pairs(2)
    rc, rg = TS._reference(pg, ctx, dim, rows, seven, pi, pj)
    nc, ng = _counts_np(dim, rows, seven, pi, pj)
    assert np.array_equal(rc, nc) and np.array_equal(rg, ng) and len({(c.tobytes(), g.tobytes()) for c, g in zip(rc, rg)}) == 7
    which = np.arange(nrep) % 7
    counts, gaps = ctx.prealigned_counts_resampled(dim, rows, np.ascontiguousarray(seven[which]), pi, pj)
    assert np.array_equal(counts, rc[which]) and np.array_equal(gaps, rg[which])


# ---- 6: the driver above the caps ---------------------------------------------------------------------------------------------------------
def test_driver_default_route_above_the_caps(oracle_build, tmp_path):
    """`-T -i 0 --bootstrap 2` with the transfer and taxon outputs on 1040 sequences, no PGM_DEVICE_* or PGM_HOST_* switch: the product
    driver's default route (BioNJ, transfer and taxa on the device from 256 taxa on) against the oracle driver's host loops; stdout and
    every file byte for byte.  Each run is a child process under a time limit of its own."""
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    n, L, seed = SR.DRIVER_FAMILY
    assert n - (SR.BIONJ_PAST - 1) > SR.BIONJ_CHUNK and n > SR.SLAB
    fa = str(tmp_path / "big.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta(gen.gen(n, L, seed)))
    env = {k: v for k, v in os.environ.items() if not (k.startswith("PGM_DEVICE_") or k.startswith("PGM_HOST_"))}

    def run(exe, tag):
        p = {k: os.path.join(str(tmp_path), "%s.%s" % (tag, k)) for k in ("out", "tbe", "taxa", "joins")}
        r = bu.run(exe, ["-T", "-i", "0", "--stats", "--bootstrap", "2", "--bootstrap_out", p["out"], "--bootstrap_tbe", p["tbe"], "--bootstrap_taxa", p["taxa"],
                         "--dump_joins", p["joins"], fa], env, timeout=240)
        return r.stdout, {k: open(v, "rb").read() for k, v in p.items()}, bu.stats_of(r.stderr)

    ref_out, ref_files, ref_st = run(os.path.join(oracle_build, "pgmsa_oracle"), "ref")
    assert ref_st["backend"] == "oracle" and ref_st["bionj_device_calls"] == 0 and len(ref_out) > 0 and all(len(v) > 0 for v in ref_files.values())
    out, files, st = run(pg.PGMSA_PATH, "hip")
    assert st["backend"] == "hip" and st["switches"] == "", st
    assert st["bionj_device_calls"] > 0 and st["bionj_launches"] > 0, st
    assert st["bootstrap_transfer_kernel_ms"] > 0 and st["bootstrap_taxa_kernel_ms"] > 0, st
    assert out == ref_out
    for k in ref_files:
        assert files[k] == ref_files[k], k
