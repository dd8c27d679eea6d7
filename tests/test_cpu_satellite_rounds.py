"""The second rounds of the satellite kernels (BioNJ, transfer bootstrap, taxon instability, WLS pair sums, gap parsimony, gap masks,
resampled pair counts): the lists of cases that sit just past each staging piece and launch cap, and what they claim, checked on the CPU.
tests/test_gpu_satellite_rounds.py runs every list on the device.  Every cap is read from the kernel header or the launch code that
sets it, so whoever moves a cap moves the case with it (the test notes of 3.8, 3.9, 3.11, 3.13, 3.15 and 3.16).

1. BioNJ: PGM_BIONJ_CHUNK elements of a column are staged in LDS at a time.  BIONJ_N = chunk + 16 taxa: the joins 0..15 have dim
   chunk + 16 .. chunk + 1 (every residue of dim mod 4; odd dims give both parities of `start` within one join), so the chunk loops
   of the sums and the join kernel take a second lap at step 0 and at steps > 0.  The families of a call go to blockIdx.y up to
   GRID_Y = 65535 and to blockIdx.z beyond: BIONJ_FAMILIES = GRID_Y + 4 small families.
2. Transfer bootstrap and taxon instability: PGM_TRANSFER_K 32-bit words (SLAB = 32 K leaves) per staged slab; the leaf counts
   SLAB / 2 + 1 (the clamp loop's second lap over 16 threads), SLAB - 1 and SLAB (one full slab), SLAB + 1 (a second slab of two
   words), 2 SLAB + 1 (a third).  The replicates go to blockIdx.y up to GRID_Y: TRANSFER_REPS = GRID_Y + 2.
3. WLS pair sums: a lane of pgm_wls_jobs_kernel adds the partials of the blocks lane, lane + 64, ... of PGM_WLS_ROWS rows each:
   WLS_N = 65 blocks + 1 row.  A launch takes the jobs whose block partials fit the 64 MB budget: WLS_JOBS = that chunk + 3.
4. Gap parsimony: a lane owns the blocks (of 32 columns) lane, lane + 256, ...: PARS_SHAPES have 257, 258 and 514 blocks.  The grid
   is the number of candidates whose consensus scratch fits the 256 MB budget: one candidate of PARS_BIG rows x columns brings it
   below the PARS_SMALL + 2 jobs of the call.  Gap masks: one workgroup per job up to GRID_Y: GAPMASK_JOBS = GRID_Y + 5.
5. Resampled pair counts: blocks of four pairs up to eight per CU, the replicates on blockIdx.y up to GRID_Y.

The third chunk of BioNJ (2049 taxa and more) is deliberately left out: the numpy statement takes 5 to 6 s per matrix at 1040 taxa and
about a minute at 2049, and the chunk loops are generic in k0 (nothing in them distinguishes the second lap from a later one)."""
import functools
import os
import random
import re

import numpy as np

import bionj_ref as B
import gen
import taxa_ref as X
import test_cpu_bionj as CB
import test_gpu_bionj as TB
import test_gpu_transfer as TG
import topology_ref as TP
import transfer_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prographmsa_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(header, name):
    """#define `name` of a kernel header."""
    return int(re.search(r"^#define %s\s+(\d+)" % name, source(header), re.M).group(1))


def found(name, pattern):
    """The one number `pattern` captures in a source file of csrc/ (a launch cap that is a literal there)."""
    hits = re.findall(pattern, source(name))
    assert len(set(hits)) == 1, (name, pattern, hits)
    return int(hits[0])


GRID_Y = 65535   # the y and z range of a grid: the cap of every launch below that deals families, replicates or jobs to blockIdx.y

# ---- 1: BioNJ ----------------------------------------------------------------------------------------------------------------------------
BIONJ_CHUNK = constant("pgm_bionj_kernels.h", "PGM_BIONJ_CHUNK")
BIONJ_PAST = 16                      # joins with dim > PGM_BIONJ_CHUNK
BIONJ_N = BIONJ_CHUNK + BIONJ_PAST   # 1040 taxa at a chunk of 1024
BIONJ_KINDS = ("asym", "lambda")     # of bionj_ref.matrices, seed 0 (test_bionj_lambdas_are_inside_the_clamp is what the seed has to meet)
BIONJ_MULTI = [("asym", BIONJ_N), ("ties", 5), ("lambda", BIONJ_N), ("random", 130)]
BIONJ_FAMILIES = GRID_Y + 4          # gz = 2: four families on blockIdx.z = 1
BIONJ_SMALL_NS = (4, 5, 6, 4, 6, 5, 4)
BIONJ_SMALL_KINDS = ("random", "asym", "ties", "ints", "tiny", "lambda", "random")
DRIVER_FAMILY = (BIONJ_N, 60, 11)    # gen.gen(n, L, seed): the family of the CPU pin and of the driver run above the caps


def bionj_case(kind):
    """(D, V, joins, final_d, info) at BIONJ_N taxa: tests/test_gpu_bionj.case, computed once per process."""
    return TB.case(kind, BIONJ_N)


@functools.lru_cache(maxsize=None)
def bionj_small():
    """The seven distinct small families of the call of BIONJ_FAMILIES: [(D, V, joins, final_d)] by the criterion and
    [(D, V, plan, joins, final_d)] by the plans of tests/topology_ref.py; family f of the call is number f % 7."""
    crit, plan = [], []
    for k, (n, kind) in enumerate(zip(BIONJ_SMALL_NS, BIONJ_SMALL_KINDS)):
        D, V = B.matrices(kind, n, seed=k)
        joins, final_d, _ = B.bionj_joins(D, V)
        crit.append((D, V, joins, final_d))
        pl = TP.plan(TP.PLANS[k % len(TP.PLANS)], n, seed=k)
        joins, final_d, _ = TP.bionj_joins_plan(D, V, pl)
        plan.append((D, V, pl, joins, final_d))
    return crit, plan


def tiled_families(per_family, nfam):
    """The arrays of family f % 7 for f < nfam, back to back (flattened)."""
    period = np.concatenate([np.asarray(a).reshape(-1) for a in per_family])
    total = sum(np.asarray(per_family[f % len(per_family)]).size for f in range(nfam % len(per_family)))
    total += (nfam // len(per_family)) * period.size
    return np.ascontiguousarray(np.tile(period, nfam // len(per_family) + 1)[:total])


# ---- 2: transfer bootstrap, taxon instability ---------------------------------------------------------------------------------------------
TRANSFER_K = constant("pgm_transfer_kernels.h", "PGM_TRANSFER_K")
SLAB = 32 * TRANSFER_K   # leaves of one staged slab
TRANSFER_LEAVES = (SLAB // 2 + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1)
TRANSFER_NREF = 65
TRANSFER_COUNTS = (66, 0, 130)   # sets of the three replicates
TRANSFER_NEAR = 40               # the first sets of replicate 0: reference set k with its high leaves flipped
TRANSFER_THR = 7                 # counts exactly the near sets (every other set is hundreds of leaves away)
TRANSFER_REPS = GRID_Y + 2       # two workgroups of blockIdx.y take a second replicate
TRANSFER_REPS_LEAVES, TRANSFER_REPS_REF = 5, [0b00011, 0b01100]


def high_leaves(n, rng):
    """The leaves a near set differs in: leaf SLAB alone at SLAB + 1 leaves, seven leaves of the later slabs beyond that; up to one
    slab the last leaf (there is no later slab)."""
    if n <= SLAB:
        return [n - 1]
    return [SLAB] if n == SLAB + 1 else sorted(rng.sample(range(SLAB, n), 7))


@functools.lru_cache(maxsize=None)
def transfer_case(n):
    """dict(ref, reps, flipped, thr, phi, taxa) at n leaves; phi is tests/transfer_ref.phi_matrix, taxa tests/taxa_ref.taxa_matrices
    (phi, arg, moved, counted); computed once per process."""
    rng = random.Random(7000 + n)
    ref = TG.bit_sets(n, TRANSFER_NREF, rng, True)
    flipped = [high_leaves(n, rng) for _ in range(TRANSFER_NEAR)]
    near = [ref[k] ^ sum(1 << t for t in flipped[k]) for k in range(TRANSFER_NEAR)]
    reps = [near + TG.bit_sets(n, TRANSFER_COUNTS[0] - TRANSFER_NEAR, rng, False)] + [TG.bit_sets(n, c, rng, False) for c in TRANSFER_COUNTS[1:]]
    thr = [TRANSFER_THR] * TRANSFER_NREF
    return dict(ref=ref, reps=reps, flipped=flipped, thr=thr, phi=T.phi_matrix(n, ref, reps), taxa=X.taxa_matrices(n, ref, thr, reps))


@functools.lru_cache(maxsize=None)
def transfer_reps_case():
    """TRANSFER_REPS replicates over five leaves, replicate k of k % 3 sets: dict(ref, reps, thr, phi, taxa)."""
    rng = random.Random(7)
    n, ref = TRANSFER_REPS_LEAVES, TRANSFER_REPS_REF
    reps = [[rng.getrandbits(n) for _ in range(k % 3)] for k in range(TRANSFER_REPS)]
    reps[1], reps[GRID_Y + 1] = [0b00110], [ref[0]]   # one workgroup's two replicates: reference set 0 is absent from the first, present in the second
    thr = [1, 0]
    return dict(ref=ref, reps=reps, thr=thr, phi=T.phi_matrix(n, ref, reps), taxa=X.taxa_matrices(n, ref, thr, reps))


# ---- 3: WLS pair sums ---------------------------------------------------------------------------------------------------------------------
WLS_ROWS = constant("pgm_wls_kernels.h", "PGM_WLS_ROWS")
WLS_SLOTS = constant("pgm_wls_kernels.h", "PGM_WLS_SLOTS")
WLS_LANES = 64                                                                  # pgm_wls_jobs_kernel: one wavefront per job
WLS_BUDGET = found("pgm_wls_capi.inc", r"\((\d+)ull << 20\) / part_job") << 20   # bytes of block partials per launch
WLS_N = WLS_ROWS * (WLS_LANES + 1) + 1                                          # 66 blocks: lanes 0 and 1 take a second one


def wls_blocks(n):
    return -(-n // WLS_ROWS)


def wls_chunk(n):
    """Jobs per launch of pgm_wls_pair_sums_batch at n rows."""
    return WLS_BUDGET // (wls_blocks(n) * WLS_SLOTS * 8)


WLS_JOBS = wls_chunk(WLS_N) + 3   # a second pair of launches, of three jobs

# ---- 4: gap parsimony, gap masks ----------------------------------------------------------------------------------------------------------
PARS_LANES = found("pgm_parsimony_capi.inc", r"pgm_gap_parsimony_kernel, dim3\(grid\), dim3\((\d+)\)")   # threads of a candidate's workgroup
PARS_COLS = 32                                                                                            # columns of a block
PARS_SHAPES = [(3, PARS_COLS * PARS_LANES + 1), (64, PARS_COLS * (PARS_LANES + 1) + 1), (5, PARS_COLS * (2 * PARS_LANES + 1) + 1)]   # (nleaves, ncols)
PARS_BUDGET = found("pgm_parsimony_capi.inc", r"budget = \((\d+)ull << 20\) / 8") << 20                  # bytes of consensus scratch
PARS_BIG = (1024, 4097)
PARS_SMALL = 300                                                                                          # jobs of 3..5 rows, 33..72 columns behind it


def pars_blocks(ncols):
    return -(-ncols // PARS_COLS)


def pars_grid(shapes):
    """Workgroups of pgm_gap_parsimony_batch for jobs of these (nleaves, ncols)."""
    per_wg = max(1, max((nl - 2) * pars_blocks(L) for nl, L in shapes))
    return max(1, min(len(shapes), PARS_BUDGET // 8 // per_wg, GRID_Y))


def pars_budget_shapes():
    """The shapes of the scratch-budget call: PARS_BIG, PARS_SMALL small jobs, and PARS_SHAPES[1] at the index that is the grid of
    the call, so that workgroup 0 walks the large job and then that one over the same scratch."""
    rng = random.Random(41)
    shapes = [PARS_BIG] + [(rng.randint(3, 5), rng.randint(33, 72)) for _ in range(PARS_SMALL)]
    at = pars_grid(shapes + [PARS_SHAPES[1]])
    shapes.insert(at, PARS_SHAPES[1])
    return shapes, at


GAPMASK_JOBS = GRID_Y + 5

# ---- 5: resampled pair counts -------------------------------------------------------------------------------------------------------------
RESAMPLE_BLOCKS_PER_CU = found("pgm_dist_capi.inc", r"multiProcessorCount \* (\d+)u\);\s*hipLaunchKernelGGL\(pgm_prealigned_resampled_kernel")
RESAMPLE_PAIRS = 4             # pairs of a workgroup: one per wavefront
RESAMPLE_L, RESAMPLE_DIM = 65, 4
RESAMPLE_REPS = GRID_Y + 2
MI355X_CUS = 256


def resample_rows(cus):
    """The smallest number of rows whose pairs are more than one round of the grid and three more."""
    n = 2
    while n * (n - 1) // 2 <= RESAMPLE_PAIRS * RESAMPLE_BLOCKS_PER_CU * cus + 3:
        n += 1
    return n


# ---- the lists hold what they claim ---------------------------------------------------------------------------------------------------------
def test_launch_caps_are_where_the_lists_expect_them():
    """Every launch that deals its work to blockIdx.y (or x, for the job kernels) stops at GRID_Y there."""
    assert found("pgm_bionj_capi.inc", r"gy = std::min\(nfam, (\d+)u\)") == GRID_Y
    assert found("pgm_transfer_capi.inc", r"std::min<uint32_t>\(nrep, (\d+)\)") == GRID_Y
    assert found("pgm_transfer_taxa_capi.inc", r"std::min<uint32_t>\(nrep, (\d+)\)") == GRID_Y
    assert found("pgm_parsimony_capi.inc", r"std::min<uint32_t>\(njobs, (\d+)u\)") == GRID_Y
    assert found("pgm_dist_capi.inc", r"std::min<uint32_t>\(nrep, (\d+)u\)") == GRID_Y
    assert found("pgm_wls_capi.inc", r"pgm_wls_jobs_kernel, dim3\(nj\), dim3\((\d+)\)") == WLS_LANES
    assert "b += blockDim.x" in source("pgm_parsimony_kernels.h") and "(j.ncols + 31) / 32" in source("pgm_parsimony_capi.inc")
    assert found("pgm_dist_capi.inc", r"\(npairs \+ 3\) / (\d+), \(uint32_t\)ctx->prop") == RESAMPLE_PAIRS


def test_bionj_sizes_lie_past_the_chunk():
    dims = [BIONJ_N - s for s in range(BIONJ_PAST)]
    assert min(dims) == BIONJ_CHUNK + 1 and {d % 4 for d in dims} == {0, 1, 2, 3}
    assert BIONJ_N - BIONJ_PAST == BIONJ_CHUNK        # join 16 is the first of one lap
    assert BIONJ_N < 2 * BIONJ_CHUNK                  # (no third lap: see the module's docstring)
    odd_pairs, tails, accumulated = set(), set(), set()   # dims whose second lap holds the odd last pair, the tail, accumulated elements
    for d in dims:
        starts = {(j * d) & 1 for j in range(d)}
        assert starts == ({0, 1} if d % 2 else {0})
        for start in starts:
            end2, end = start + ((d - start) // 4) * 4, start + ((d - start) // 2) * 2
            if end > end2 >= BIONJ_CHUNK: odd_pairs.add(d)
            if end < d: tails.add(d)   # (element d - 1 >= chunk)
            if end2 > BIONJ_CHUNK: accumulated.add(d)
    assert len(odd_pairs) >= 4 and len(tails) >= 8 and len(accumulated) >= 15
    assert [n for _, n in BIONJ_MULTI] == [BIONJ_N, 5, BIONJ_N, 130] and {k for k, n in BIONJ_MULTI if n == BIONJ_N} == set(BIONJ_KINDS)
    assert DRIVER_FAMILY[0] == BIONJ_N


def test_bionj_lambdas_are_inside_the_clamp():
    """At least 8 of the 16 joins with dim > PGM_BIONJ_CHUNK have 0 < lambda < 1, for either kind: a wrong vsum in the join kernel's
    second lap then changes the new row, not only a value the clamp hides.  (`lambda` at seed 0: exactly 8; `asym`: all 16.)"""
    for kind in BIONJ_KINDS:
        D, V, joins, final_d, info = bionj_case(kind)
        lam = info["lambda"]
        assert lam.shape == (BIONJ_N - 3,) and len(joins) == BIONJ_N - 3
        first = lam[:BIONJ_PAST]
        assert int(((first > 0.0) & (first < 1.0)).sum()) >= 8, (kind, first)
        inside = (lam > 0.0) & (lam < 1.0)
        assert info["lambda_at_0"] == int((lam < 0.0).sum()) and info["lambda_at_1"] == int((lam > 1.0).sum())
        assert inside.sum() + info["lambda_at_0"] + info["lambda_at_1"] + int(np.isnan(lam).sum()) + int(((lam == 0.0) | (lam == 1.0)).sum()) == len(lam)
    assert bionj_case("lambda")[4]["lambda_at_0"] > 0 and bionj_case("lambda")[4]["lambda_at_1"] > 0


def test_bionj_statement_is_the_host_loop_above_the_chunk(oracle_build, tmp_path):
    """The numpy statement against the host loop at BIONJ_N taxa, on the dumped matrices of the oracle driver, bit for bit: which of
    the two a device mismatch above the chunk would be measured against."""
    n, L, seed = DRIVER_FAMILY
    fa = tmp_path / "big.fa"
    fa.write_text(gen.fasta(gen.gen(n, L, seed)))
    out, dists, joins = CB.dump_run(os.path.join(oracle_build, "pgmsa_oracle"), ["-T", "-i", "0"], fa, tmp_path, "big")
    assert len(dists) == 1 and dists[0][0].shape == (n, n) and joins[0][0] == n and len(out) > 0
    CB.assert_statement(dists, joins)


def test_bionj_small_families():
    crit, plan = bionj_small()
    assert len(crit) == len(plan) == len(BIONJ_SMALL_NS) == 7
    assert len({(D.tobytes(), V.tobytes()) for D, V, _, _ in crit}) == 7
    assert GRID_Y % 7 == 1 and BIONJ_FAMILIES - GRID_Y == 4   # family f and family f - GRID_Y (the same blockIdx.y) never share a matrix
    assert all(f % 7 != (f - GRID_Y) % 7 for f in range(GRID_Y, BIONJ_FAMILIES))
    assert [len(j) for _, _, j, _ in crit] == [n - 3 for n in BIONJ_SMALL_NS]
    assert any(not B.same_bits(c[2], p[3]) for c, p in zip(crit, plan))   # (the plans are not the criterion's joins)
    for (D, V, pl, joins, _), n in zip(plan, BIONJ_SMALL_NS):
        assert TP.read_plan_joins(joins) == pl[:n - 3]
    tiled = tiled_families([j for _, _, j, _ in crit], 16)   # two periods of 13 joins, then the families 0 and 1 once more
    assert len(tiled) == 2 * 13 + 1 + 2 and B.same_bits(tiled[26:27], crit[0][2]) and B.same_bits(tiled[27:29], crit[1][2])
    assert B.same_bits(tiled_families([f for _, _, _, f in crit], BIONJ_FAMILIES)[-9:], crit[(BIONJ_FAMILIES - 1) % 7][3].reshape(-1))


def test_transfer_leaf_counts():
    words32 = [2 * ((n + 63) // 64) for n in TRANSFER_LEAVES]
    k = TRANSFER_K
    assert words32 == [k // 2 + 2, k, k, k + 2, 2 * k + 2]
    assert words32[0] > 16                                              # the clamp's popcount loop: 16 threads, a second lap
    assert [-(-w // k) for w in words32] == [1, 1, 1, 2, 3]             # slabs
    assert TRANSFER_COUNTS[0] > 64 > TRANSFER_NEAR and TRANSFER_NREF > 64
    assert TRANSFER_REPS - GRID_Y == 2


def test_transfer_high_leaves_decide():
    """The first 40 sets of replicate 0 differ from reference set k in leaves of the later slabs only, and nothing else is near: phi
    is 1 (SLAB + 1 leaves) or 7 (2 SLAB + 1) there, the arg-min is set k, the moved leaves are those leaves and only those pairs are
    counted.  The statement on the first slab alone (every leaf >= SLAB masked off) differs in each of those 40 entries: a kernel
    that drops a later slab cannot pass."""
    mask = (1 << SLAB) - 1
    for n in TRANSFER_LEAVES:
        case = transfer_case(n)
        phi, (tphi, arg, moved, counted) = case["phi"], case["taxa"]
        assert [len(r) for r in case["reps"]] == list(TRANSFER_COUNTS) and tphi == phi
        want = 7 if n > SLAB + 1 else 1
        for k in range(TRANSFER_NEAR):
            assert phi[k][0] == want == len(case["flipped"][k]) and arg[k][0] == k
            assert [t for t in range(n) if moved[k][t]] == case["flipped"][k] and max(moved[k]) == 1
            assert n <= SLAB or min(case["flipped"][k]) >= SLAB
        assert counted == [1] * TRANSFER_NEAR + [0] * (TRANSFER_NREF - TRANSFER_NEAR)
        assert all(phi[e][r] > TRANSFER_THR for e in range(TRANSFER_NREF) for r in range(3) if (e >= TRANSFER_NEAR or r > 0))
        assert all(phi[e][1] == T.p_of(case["ref"][e], n) - 1 for e in range(TRANSFER_NREF))   # (the replicate without a set: the clamp)
        if n > SLAB:
            first_slab = T.phi_matrix(SLAB, [a & mask for a in case["ref"]], [[b & mask for b in r] for r in case["reps"]])
            assert all(first_slab[k][0] == 0 for k in range(TRANSFER_NEAR))
            assert sum(first_slab[e][r] != phi[e][r] for e in range(TRANSFER_NREF) for r in range(3)) >= TRANSFER_NEAR
    assert transfer_case(SLAB + 1)["flipped"] == [[SLAB]] * TRANSFER_NEAR


def test_transfer_many_replicates():
    case = transfer_reps_case()
    assert [len(r) for r in case["reps"][:6]] == [0, 1, 2, 0, 1, 2] and len(case["reps"]) == TRANSFER_REPS > GRID_Y
    phi, arg, moved, counted = case["taxa"]
    assert phi == case["phi"] and len(phi[0]) == TRANSFER_REPS
    assert (phi[0][1], phi[0][GRID_Y + 1]) == (1, 0) and (arg[0][GRID_Y], arg[0][GRID_Y + 1]) == (X.NONE, sum(k % 3 for k in range(GRID_Y + 1)))   # (the second round is no copy of the first)
    assert 0 < counted[1] < counted[0] < TRANSFER_REPS and sum(moved[0]) > 0


def test_wls_grid_is_smaller_than_the_jobs():
    assert wls_blocks(WLS_N) == WLS_LANES + 2 and wls_blocks(WLS_N - 1) == WLS_LANES + 1
    chunk = wls_chunk(WLS_N)
    assert chunk * wls_blocks(WLS_N) * WLS_SLOTS * 8 <= WLS_BUDGET < (chunk + 1) * wls_blocks(WLS_N) * WLS_SLOTS * 8
    assert chunk < WLS_JOBS == chunk + 3 and 2 * -(-WLS_JOBS // chunk) == 4          # four launches
    assert WLS_JOBS * (WLS_N * 9) < 80 << 20                                           # (labels and offsets of the call: some 60 MB)


def test_parsimony_grid_is_smaller_than_the_jobs():
    assert [pars_blocks(L) for _, L in PARS_SHAPES] == [PARS_LANES + 1, PARS_LANES + 2, 2 * PARS_LANES + 2]
    assert all(L % PARS_COLS == 1 for _, L in PARS_SHAPES)
    shapes, at = pars_budget_shapes()
    grid = pars_grid(shapes)
    per_wg = (PARS_BIG[0] - 2) * pars_blocks(PARS_BIG[1])
    assert grid == at == PARS_BUDGET // 8 // per_wg < len(shapes) == PARS_SMALL + 2
    assert shapes[0] == PARS_BIG and shapes[grid] == PARS_SHAPES[1] and grid < GRID_Y
    assert all(nl <= 5 and 33 <= L <= 72 for k, (nl, L) in enumerate(shapes) if k not in (0, grid))
    assert 8 * per_wg * grid <= PARS_BUDGET < 1 << 29                                 # (device memory of the case: below 0.5 GB)
    assert pars_blocks(shapes[grid][1]) != pars_blocks(PARS_BIG[1])                   # another block stride over the same scratch
    assert GAPMASK_JOBS - GRID_Y == 5


def test_resample_sizes():
    n = resample_rows(MI355X_CUS)
    one_round = RESAMPLE_PAIRS * RESAMPLE_BLOCKS_PER_CU * MI355X_CUS
    assert n * (n - 1) // 2 > one_round + 3 >= (n - 1) * (n - 2) // 2
    assert RESAMPLE_REPS - GRID_Y == 2 and GRID_Y % 7 != 0   # (replicate r draws column vector r % 7: never that of replicate r - GRID_Y)
