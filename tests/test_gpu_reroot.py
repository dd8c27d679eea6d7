"""Root search on the MI355X: the gap mask and gap parsimony kernels against numpy, and `pgmsa -r` / `-rr` against the CPU
oracle driver and against the independent statement of tests/test_cpu_reroot.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gen
import test_cpu_reroot as R

GOLD = R.GOLD
pytestmark = pytest.mark.gpu


def _P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def pack(gaps):
    """nrows x ncols bool -> nrows x ceil(ncols / 64) uint64 (bit c % 64 of word c / 64)."""
    nr, nc = gaps.shape
    W = (nc + 63) // 64
    if W == 0:
        return np.zeros((max(nr, 1), 1), np.uint64)
    pad = np.zeros((nr, W * 64), bool)
    pad[:, :nc] = gaps
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view("<u8").reshape(nr, W))


def parsimony_np(gaps, children):
    """tests/test_cpu_reroot.gap_parsimony, vectorised over the blocks (the same bits)."""
    nl, L = gaps.shape
    nb = (L + 31) // 32
    valid = np.zeros(nb * 32, bool)
    valid[:L] = True
    if L % 32 == 0:
        valid[L - 32:] = False   # the padding loop's quirk
    g = np.zeros((nl, nb * 32), bool)
    g[:, :L] = gaps
    res = (~g & valid) | ~valid
    gap = (g & valid) | ~valid
    res = res.reshape(nl, nb, 32).astype(np.uint64)
    gap = gap.reshape(nl, nb, 32).astype(np.uint64)
    sh = np.arange(32, dtype=np.uint64)
    leaf = ((res << (2 * sh)) | (gap << (2 * sh + np.uint64(1)))).sum(axis=2, dtype=np.uint64)
    cons = list(leaf) + [None] * (nl - 1)
    score = 0
    HI = np.uint64(0xAAAAAAAAAAAAAAAA)
    for k, (a, b) in enumerate(children):
        x = cons[a] & cons[b]
        t = ~x
        t = t & (t << np.uint64(1)) & HI
        score += int(np.bitwise_count(t).sum())
        cons[nl + k] = x | t | (t >> np.uint64(1))
    return score


def random_topology(rng, nl):
    avail = list(range(nl))
    ch = []
    while len(avail) > 1:
        i, j = sorted(rng.choice(len(avail), 2, replace=False))
        a, b = avail[i], avail[j]
        del avail[j], avail[i]
        ch.append((a, b) if rng.random() < 0.5 else (b, a))
        avail.append(nl + len(ch) - 1)
    return ch


def run_parsimony(ctx, cands):
    import prographmsa_amd as pg
    keep, jobs = [], (pg.pgm_parsimony_job * len(cands))()
    for i, (gaps, ch) in enumerate(cands):
        m = pack(gaps)
        c = np.ascontiguousarray(np.array(ch, np.uint32).reshape(-1))
        keep += [m, c]
        jobs[i].masks = _P(m, C.c_uint64); jobs[i].children = _P(c, C.c_uint32)
        jobs[i].nleaves = gaps.shape[0]; jobs[i].ncols = gaps.shape[1]
    scores = np.zeros(len(cands), np.uint32)
    rc = pg.lib.pgm_gap_parsimony_batch(ctx.handle, len(cands), jobs, _P(scores, C.c_uint32))
    return rc, scores


def test_numpy_restatements_agree():
    rng = np.random.default_rng(1)
    for nl, L in [(2, 1), (3, 31), (5, 32), (7, 33), (9, 64), (6, 65), (4, 100)]:
        g = rng.random((nl, L)) < 0.3
        t = random_topology(rng, nl)
        assert parsimony_np(g, t) == R.gap_parsimony(g, t)


@pytest.mark.parametrize("nl", [2, 3, 64, 1024])
def test_gap_parsimony_kernel(ctx, nl):
    import prographmsa_amd as pg
    rng = np.random.default_rng(nl)
    cands = []
    for L in [1, 31, 32, 33, 3274, 4096]:
        for rep in range(3 if nl < 1024 else 1):
            g = rng.random((nl, L)) < rng.choice([0.05, 0.3, 0.7])
            cands.append((g, random_topology(rng, nl)))
    rc, scores = run_parsimony(ctx, cands)
    pg.check(rc)
    assert [int(s) for s in scores] == [parsimony_np(g, t) for g, t in cands]


def test_gap_parsimony_kernel_many_candidates(ctx):
    """One launch, 509 candidates of one 256-row family (the headline's count), rows permuted per candidate."""
    import prographmsa_amd as pg
    rng = np.random.default_rng(5)
    base = rng.random((256, 1500)) < 0.2
    cands = [(base[rng.permutation(256)], random_topology(rng, 256)) for _ in range(509)]
    rc, scores = run_parsimony(ctx, cands)
    pg.check(rc)
    assert [int(s) for s in scores] == [parsimony_np(g, t) for g, t in cands]


def test_gap_parsimony_rejects_bad_input(ctx):
    import prographmsa_amd as pg
    g = np.zeros((4, 40), bool)
    ok = [(0, 1), (2, 3), (4, 5)]
    for gg, ch in [(g[:1], [(0, 0)]),                  # fewer than two rows
                   (g[:, :0], ok),                     # no columns
                   (g, [(0, 1), (2, 9), (4, 5)]),      # child out of range
                   (g, [(0, 1), (2, 5), (4, 3)]),      # not in post-order (node 1 reads itself)
                   (g, [(0, 1), (0, 3), (4, 5)])]:     # a row under two nodes
        rc, _ = run_parsimony(ctx, [(gg, ch)])
        assert rc == pg.PGM_ERR_INVALID, (ch, gg.shape)
    rc, _ = run_parsimony(ctx, [(g, ok)])
    assert rc == pg.PGM_OK


def _extend_np(child, mapping):
    out = np.ones((child.shape[0], len(mapping)), bool)
    k = 0
    for j, m in enumerate(mapping):
        if m != 0xFFFFFFFF:
            out[:, j] = child[:, k]
            k += 1
    return out


def test_gapmask_extend_kernel(ctx):
    import prographmsa_amd as pg
    rng = np.random.default_rng(3)
    cases = []
    for nrows, nin, nout in [(1, 1, 1), (1, 5, 70), (3, 64, 64), (17, 63, 130), (256, 1000, 1500), (40, 0, 33), (5, 200, 4097)]:
        child = rng.random((nrows, nin)) < 0.3
        pos = np.sort(rng.choice(nout, nin, replace=False))
        mapping = np.full(nout, 0xFFFFFFFF, np.uint32)
        mapping[pos] = np.arange(1, nin + 1, dtype=np.uint32)
        cases.append((child, mapping))
    jobs = (pg.pgm_gapmask_job * len(cases))()
    keep, outs = [], []
    for i, (child, mapping) in enumerate(cases):
        src = pack(child) if child.shape[1] else np.zeros((child.shape[0], 1), np.uint64)
        dst = np.full((child.shape[0], (len(mapping) + 63) // 64), 0xDEAD, np.uint64)
        keep += [src, mapping]
        outs.append(dst)
        jobs[i].src = _P(src, C.c_uint64); jobs[i].mapping = _P(mapping, C.c_uint32); jobs[i].dst = _P(dst, C.c_uint64)
        jobs[i].nrows = child.shape[0]; jobs[i].ncols_in = child.shape[1]; jobs[i].ncols_out = len(mapping)
    pg.check(pg.lib.pgm_gapmask_extend_batch(ctx.handle, len(cases), jobs))
    for (child, mapping), dst in zip(cases, outs):
        assert np.array_equal(dst, pack(_extend_np(child, mapping)))
    # the mapping must cover the child's columns exactly
    bad = cases[2][1].copy()
    bad[np.nonzero(bad != 0xFFFFFFFF)[0][0]] = 0xFFFFFFFF
    jobs[2].mapping = _P(bad, C.c_uint32)
    assert pg.lib.pgm_gapmask_extend_batch(ctx.handle, len(cases), jobs) == pg.PGM_ERR_INVALID


def _both(oracle_build, args, cwd=None):
    import prographmsa_amd as pg
    out = []
    for exe in (pg.PGMSA_PATH, os.path.join(oracle_build, "pgmsa_oracle")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=cwd)
        assert r.returncode == 0, (exe, r.stderr)
        out.append((r.stdout, [ln for ln in r.stderr.splitlines() if ln.startswith("best gap parsimony score: ")]))
    assert out[0][1] and len(out[0][1]) == 1
    return out


@pytest.mark.parametrize("flag", ["-r", "-rr"])
@pytest.mark.parametrize("case", ["c2_tree", "c2_default", "cd1_codon", "c1_cs_iter"])
def test_pgmsa_reroot_equals_oracle(oracle_build, case, flag):
    g = lambda f: os.path.join(GOLD, f)
    args = {"c2_tree": ["-t", g("c2.tree"), g("c2.fa")],
            "c2_default": [g("c2.fa")],
            "cd1_codon": ["--codon", "-t", g("cd1.tree"), g("cd1.fa")],
            "c1_cs_iter": ["-c", g("K50.lib"), "-i", "1", "-t", g("c1.tree"), g("c1.fa")]}[case]
    prod, orac = _both(oracle_build, ["-f", flag] + args)
    assert prod == orac


def test_pgmsa_reroot_with_repeats_equals_oracle(oracle_build, tmp_path):
    seqs, trd = gen.gen_repeat_family(12, 120, 11)
    (tmp_path / "r.fa").write_text(gen.fasta(seqs)); (tmp_path / "r.trd").write_text(trd)
    for flag in ("-r", "-rr"):
        prod, orac = _both(oracle_build, ["-f", flag, "--read_repeats", str(tmp_path / "r.trd"), str(tmp_path / "r.fa")])
        assert prod == orac


@pytest.mark.parametrize("case", ["c1", "gen24"])
def test_pgmsa_reroot_equals_rerooted_plain_passes(oracle_build, tmp_path, case):
    import prographmsa_amd as pg
    if case == "c1":
        fa, tree = os.path.join(GOLD, "c1.fa"), open(os.path.join(GOLD, "c1.tree")).read().strip()
    else:
        fa = str(tmp_path / "g.fa")
        open(fa, "w").write(gen.fasta(gen.gen(24, 160, 9)))
        r = subprocess.run([os.path.join(oracle_build, "pgmsa_oracle"), "-T", fa], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        tree = r.stdout.strip()
    R.check_root_search(pg.PGMSA_PATH, fa, tree, tmp_path)
