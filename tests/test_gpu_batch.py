"""`pgmsa --batch` on the MI355X: the product driver against its own solo runs and against the CPU oracle driver, and the two
segmented distance kernels (pgm_kmer_cosine_multi, pgm_prealigned_counts_multi) bit for bit against the per-family entry points and
the oracle library.  Every driver run is a child process under a time limit of its own."""
import ctypes as C
import os

import numpy as np
import pytest

import batch_util as bu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
P = lambda a, t: a.ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return bu.aa_families(tmp_path_factory.mktemp("batch_fams"))


@pytest.fixture(scope="module")
def trees(exe, fams, tmp_path_factory):
    return bu.solo_trees(exe, fams, [], tmp_path_factory.mktemp("batch_trees"))


FLOWS = {
    "fasta_t": (["--fasta"], True),
    "fasta": (["--fasta"], False),
    "fasta_a_m": (["--fasta", "-a", "-m"], False),
    "T_i0": (["-T", "-i", "0"], False),
    "fasta_F": (["--fasta", "-F"], False),
    "fasta_c": (["--fasta", "-c", os.path.join(GOLD, "K50.lib")], False),
}


@pytest.mark.parametrize("flow", sorted(FLOWS))
def test_batch_equals_solo(exe, fams, trees, tmp_path, flow):
    opts, with_trees = FLOWS[flow]
    t = trees if with_trees else None
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, flow, t)
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts, t))
    assert st["backend"] == "hip" and st["batch_families"] == 12 and st["batch_failed"] == 0 and st["batch_chunks"] == 1


@pytest.mark.parametrize("opts", [["--fasta"], ["--fasta", "-M", "-i", "1"]], ids=["fasta", "fasta_M_i1"])
def test_host_counts_batch_equals_solo(exe, fams, tmp_path, opts):
    """PGM_HOST_COUNTS=1 on the four smallest families (2, 2, 3 and 3 sequences: one pair and several pairs per block, and blocks that
    do not start at pair 0): the host counting loop over the pairs of all families gives every family the file of its solo run."""
    env = dict(os.environ, PGM_HOST_COUNTS="1")
    small = fams[:4]
    outs, st, _ = bu.run_batch(exe, small, opts, tmp_path, "hc%d" % len(opts), env=env)
    bu.assert_identical(outs, bu.solo_outputs(exe, small, opts, env=env))
    assert st["backend"] == "hip" and st["batch_families"] == 4 and st["batch_failed"] == 0


def test_dna_custom_model(exe, tmp_path):
    fams = bu.dna_families(tmp_path)
    opts = ["--fasta", "--dna", "--custom_model", bu.hky_model(tmp_path)]
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, "dna")
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts))
    assert st["batch_failed"] == 0


def test_batch_equals_the_oracle_batch(exe, oracle_build, fams, tmp_path):
    """The default flow: the segmented kernels of the product against the oracle backend's per-family loop (Backend's defaults)."""
    outs, _, _ = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "hip")
    ref, st, _ = bu.run_batch(os.path.join(oracle_build, "pgmsa_oracle"), fams, ["--fasta"], tmp_path, "oracle")
    assert st["backend"] == "oracle"
    for a, b in zip(outs, ref):
        assert open(a).read() == open(b).read() and len(open(a).read()) > 0


def test_committed_fixtures_reproduce_the_golden_files(exe, tmp_path):
    fams = [os.path.join(GOLD, c + ".fa") for c in ("c1", "c2")]
    trees = [os.path.join(GOLD, c + ".tree") for c in ("c1", "c2")]
    outs, st, _ = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "gold", trees)
    for o, c in zip(outs, ("c1", "c2")):
        assert open(o).read() == open(os.path.join(GOLD, c + ".out.fa")).read()


def test_distance_calls_do_not_grow_with_the_families(exe, fams, tmp_path):
    """The default flow in one chunk: one cosine call and one pair-count call per round, however many families share them."""
    a = bu.run_batch(exe, fams[:4], ["--fasta"], tmp_path, "d4")[1]
    b = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "d12")[1]
    assert a["batch_chunks"] == b["batch_chunks"] == 1
    assert a["batch_dist_calls"] == b["batch_dist_calls"] == 3
    own = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "d12own", extra=["--batch_cells", "1"])[1]
    assert own["batch_chunks"] == 12 and own["batch_dist_calls"] > 12   # (nothing shared: every family makes its own calls)


# ---- pgm_kmer_cosine_multi ------------------------------------------------------------------------------------------------
def _cosine_case(rng, nseq, ncols):
    counts = [rng.poisson(0.6, (n, ncols)).astype(np.int32) for n in nseq]
    for c in counts:
        c[:, 0] += 1   # no all-zero row
    return counts


@pytest.mark.parametrize("shape", ["five_families", "one_family", "many_small_dna"])
def test_kmer_cosine_multi_bit_identical(ctx, shape):
    import oracle_lib
    import prographmsa_amd as pg
    rng = np.random.default_rng(77)
    if shape == "five_families":
        nseq, ncols = [2, 40, 17, 16, 33], 400
    elif shape == "one_family":
        nseq, ncols = [23], 400
    else:
        nseq, ncols = [int(x) for x in rng.integers(2, 7, 300)], 4096
    counts = _cosine_case(rng, nseq, ncols)
    flat = np.ascontiguousarray(np.concatenate(counts, axis=0))
    ns = np.array(nseq, np.uint32)
    out = np.full(int(sum(n * n for n in nseq)), np.nan)
    pg.check(pg.lib.pgm_kmer_cosine_multi(ctx.handle, len(nseq), P(ns, C.c_uint32), ncols, P(flat, C.c_int32), P(out, C.c_double)))
    o = 0
    for n, c in zip(nseq, counts):
        one = np.zeros(n * n)
        pg.check(pg.lib.pgm_kmer_cosine(ctx.handle, n, ncols, P(c, C.c_int32), P(one, C.c_double)))
        assert np.array_equal(out[o:o + n * n].view(np.uint64), one.view(np.uint64))
        if shape == "five_families":
            assert np.array_equal(one.view(np.uint64), oracle_lib.kmer_cosine(c).view(np.uint64))
        o += n * n


def test_kmer_cosine_multi_invalid(ctx):
    import prographmsa_amd as pg
    counts = np.ones((5, 400), np.int32)
    out = np.zeros(25)
    ns = np.array([3, 2], np.uint32)
    f = pg.lib.pgm_kmer_cosine_multi
    assert f(ctx.handle, 2, P(ns, C.c_uint32), 400, P(counts, C.c_int32), P(out, C.c_double)) == 0
    bad = [f(None, 2, P(ns, C.c_uint32), 400, P(counts, C.c_int32), P(out, C.c_double)),
           f(ctx.handle, 2, None, 400, P(counts, C.c_int32), P(out, C.c_double)),
           f(ctx.handle, 2, P(ns, C.c_uint32), 400, None, P(out, C.c_double)),
           f(ctx.handle, 2, P(ns, C.c_uint32), 400, P(counts, C.c_int32), None),
           f(ctx.handle, 0, P(ns, C.c_uint32), 400, P(counts, C.c_int32), P(out, C.c_double)),
           f(ctx.handle, 2, P(np.array([4, 1], np.uint32), C.c_uint32), 400, P(counts, C.c_int32), P(out, C.c_double))]
    assert all(rc == pg.PGM_ERR_INVALID for rc in bad), bad


# ---- pgm_prealigned_counts_multi ------------------------------------------------------------------------------------------
def _rows(rng, dim, n, L):
    r = rng.integers(0, dim, (n, L)).astype(np.int8)
    r[rng.random((n, L)) < 0.25] = -1
    r[rng.random((n, L)) < 0.03] = -2
    return r


def _multi(pg, ctx, dim, mats, fam, pi, pj):
    nrows = np.array([m.shape[0] for m in mats], np.uint32)
    ncols = np.array([m.shape[1] for m in mats], np.uint32)
    rows = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mats]))
    counts = np.full(len(fam) * dim * dim, -7, np.int32)
    gaps = np.full(len(fam), 12345, np.uint32)
    rc = pg.lib.pgm_prealigned_counts_multi(ctx.handle, dim, len(mats), P(nrows, C.c_uint32), P(ncols, C.c_uint32), P(rows, C.c_int8), len(fam),
                                            P(fam, C.c_uint32), P(pi, C.c_uint32), P(pj, C.c_uint32), P(counts, C.c_int32), P(gaps, C.c_uint32))
    return rc, counts.reshape(len(fam), dim * dim), gaps


@pytest.mark.parametrize("dim", [4, 20, 61])
def test_prealigned_counts_multi_bit_identical(ctx, dim):
    import oracle_lib
    import prographmsa_amd as pg
    rng = np.random.default_rng(900 + dim)
    shapes = [(5, 1), (2, 63), (9, 64), (7, 65), (12, 333), (3, 1000), (6, 130)]
    mats = [_rows(rng, dim, n, L) for n, L in shapes]
    fam, pi, pj = [], [], []
    for f, (n, _) in enumerate(shapes):
        for i in range(n):
            for j in range(i + 1, n):
                fam.append(f); pi.append(i); pj.append(j)
    order = rng.permutation(len(fam))   # (the pairs of the families interleaved)
    fam = np.array(fam, np.uint32)[order]; pi = np.array(pi, np.uint32)[order]; pj = np.array(pj, np.uint32)[order]
    rc, counts, gaps = _multi(pg, ctx, dim, mats, fam, pi, pj)
    assert rc == 0
    Dk = max(dim, 20)   # (the per-family entry point takes 20 to 64 states: a smaller matrix is the corner of its 20 x 20)
    for f, m in enumerate(mats):
        sel = np.nonzero(fam == f)[0]
        qi = np.ascontiguousarray(pi[sel]); qj = np.ascontiguousarray(pj[sel])
        c = np.zeros(len(sel) * Dk * Dk, np.int32); g = np.zeros(len(sel), np.uint32)
        pg.check(pg.lib.pgm_prealigned_counts_batch(ctx.handle, Dk, m.shape[0], m.shape[1], P(m, C.c_int8), len(sel), P(qi, C.c_uint32), P(qj, C.c_uint32),
                                                    P(c, C.c_int32), P(g, C.c_uint32)))
        corner = c.reshape(len(sel), Dk, Dk)[:, :dim, :dim].reshape(len(sel), dim * dim)
        assert np.array_equal(counts[sel], corner) and np.array_equal(gaps[sel], g)
        oc, og = oracle_lib.prealigned_counts(dim, m, qi, qj)
        assert np.array_equal(counts[sel], np.asarray(oc).reshape(len(sel), dim * dim)) and np.array_equal(gaps[sel], og)


def test_prealigned_counts_multi_invalid(ctx):
    import prographmsa_amd as pg
    rng = np.random.default_rng(5)
    mats = [_rows(rng, 20, 3, 40), _rows(rng, 20, 2, 17)]
    u = lambda *v: np.array(v, np.uint32)
    assert _multi(pg, ctx, 20, mats, u(0, 1), u(0, 0), u(2, 1))[0] == 0
    bad = [_multi(pg, ctx, 20, mats, u(0, 2), u(0, 0), u(2, 1))[0],            # fam[p] >= nfam
           _multi(pg, ctx, 20, mats, u(0, 1), u(0, 0), u(2, 2))[0],            # a pair index outside its family
           _multi(pg, ctx, 20, mats, u(0, 1), u(3, 0), u(2, 1))[0],
           _multi(pg, ctx, 20, [mats[0], mats[1][:1]], u(0, 0), u(0, 0), u(1, 2))[0]]   # a family with fewer than 2 rows
    nrows = u(3, 2); ncols = u(40, 17); rows = np.concatenate([m.reshape(-1) for m in mats]); fam = u(0, 1); pi = u(0, 0); pj = u(2, 1)
    counts = np.zeros(800, np.int32); gaps = np.zeros(2, np.uint32)
    args = [ctx.handle, 20, 2, P(nrows, C.c_uint32), P(ncols, C.c_uint32), P(rows, C.c_int8), 2, P(fam, C.c_uint32), P(pi, C.c_uint32), P(pj, C.c_uint32),
            P(counts, C.c_int32), P(gaps, C.c_uint32)]
    for k in (0, 3, 4, 5, 7, 8, 9, 10, 11):   # null pointers
        a = list(args); a[k] = None
        bad.append(pg.lib.pgm_prealigned_counts_multi(*a))
    a = list(args); a[2] = 0                    # nfam == 0
    bad.append(pg.lib.pgm_prealigned_counts_multi(*a))
    assert all(rc == pg.PGM_ERR_INVALID for rc in bad), bad
