"""BioNJ on the MI355X: pgm_bionj / pgm_bionj_multi (csrc/pgm_bionj_kernels.h) against the numpy statement of tests/bionj_ref.py,
bit for bit (tests/test_cpu_bionj.py pins that statement to the host loop and the goldens), the rejections of the C ABI, and the
product driver with PGM_DEVICE_BIONJ=1 against the plain oracle driver (host loop): identical stdout and --dump_joins files.
Every driver run is a child process under a time limit of its own."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import batch_util as bu
import bionj_ref as B
import gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NW_TREES = json.load(open(os.path.join(GOLD, "nw_trees.json")))
SIZES = [4, 5, 6, 7, 8, 63, 64, 65, 130, 257]   # one join, both start parities, the 4-cluster ending, wavefront and workgroup edges
MULTI = [4, 257, 5, 64, 8, 130]
PD = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(D, V, joins, final_d, info) of one matrix kind and size; the reference is computed once and shared."""
    D, V = B.matrices(kind, n)
    joins, final_d, info = B.bionj_joins(D, V)
    for a in (D, V, joins, final_d):
        a.setflags(write=False)
    return D, V, joins, final_d, info


def device_multi(ctx, mats, expect=0):
    """pgm_bionj_multi over [(D, V)]; returns ([joins], [final_d], launches)."""
    import prographmsa_amd as pg
    ns = np.array([D.shape[0] for D, _ in mats], np.uint32)
    Dcat = np.ascontiguousarray(np.concatenate([np.asarray(D).reshape(-1) for D, _ in mats]))
    Vcat = np.ascontiguousarray(np.concatenate([np.asarray(V).reshape(-1) for _, V in mats]))
    joins = np.zeros(int((ns.astype(np.int64) - 3).clip(0).sum()) + 1, B.JOIN_DTYPE)
    final_d = np.full(9 * len(mats), -1.0)
    rc = pg.lib.pgm_bionj_multi(ctx.handle, len(mats), ns.ctypes.data_as(C.POINTER(C.c_uint32)), PD(Dcat), PD(Vcat),
                                joins.ctypes.data_as(C.POINTER(pg.pgm_bionj_join)), PD(final_d))
    assert rc == expect, (rc, pg.lib.pgm_last_error())
    out_j, o = [], 0
    for n in ns:
        out_j.append(joins[o:o + max(int(n) - 3, 0)])
        o += max(int(n) - 3, 0)
    return out_j, [final_d[9 * f:9 * f + 9].reshape(3, 3) for f in range(len(mats))], pg.lib.pgm_bionj_last_launches(ctx.handle)


def device_solo(ctx, D, V, expect=0):
    import prographmsa_amd as pg
    n = D.shape[0]
    D, V = np.ascontiguousarray(D), np.ascontiguousarray(V)
    joins = np.zeros(max(n - 3, 1), B.JOIN_DTYPE)
    final_d = np.full(9, -1.0)
    rc = pg.lib.pgm_bionj(ctx.handle, n, PD(D), PD(V), joins.ctypes.data_as(C.POINTER(pg.pgm_bionj_join)), PD(final_d))
    assert rc == expect, (rc, pg.lib.pgm_last_error())
    return joins[:max(n - 3, 0)], final_d.reshape(3, 3), pg.lib.pgm_bionj_last_launches(ctx.handle)


def assert_record(got_j, got_f, ref_j, ref_f, what):
    first = np.flatnonzero((got_j["index1"] != ref_j["index1"]) | (got_j["index2"] != ref_j["index2"]))
    assert first.size == 0, "%s: join %d is %s, the statement joins %s" % (what, first[0], got_j[first[0]], ref_j[first[0]])
    assert B.same_bits(got_j, ref_j), "%s: branch lengths differ" % (what,)
    assert B.same_bits(got_f, ref_f), "%s: final_d %s != %s" % (what, got_f, ref_f)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", B.KINDS)
def test_bionj_matches_the_statement(ctx, kind, n):
    D, V, ref_j, ref_f, info = case(kind, n)
    D0, V0 = D.copy(), V.copy()
    got_j, got_f, launches = device_solo(ctx, D, V)
    assert B.same_bits(D, D0) and B.same_bits(V, V0)   # the inputs are not modified
    assert_record(got_j, got_f, ref_j, ref_f, "%s n = %d" % (kind, n))
    assert launches > 0 and launches % (n - 3) == 0
    if kind == "lambda":   # the statement took the clamps this kind is there for: both from 7 taxa on, one of them below
        assert info["lambda_at_0"] + info["lambda_at_1"] > 0
        assert n < 7 or (info["lambda_at_0"] > 0 and info["lambda_at_1"] > 0), info
    if kind == "tiny":
        assert (D[D > 0] < B.MIN_DIST).any() and (V[V > 0] < B.MIN_VAR).any()


def test_lambda_cases_take_both_clamps():
    infos = [case("lambda", n)[4] for n in SIZES]
    assert sum(i["lambda_at_0"] for i in infos) > 0 and sum(i["lambda_at_1"] for i in infos) > 0


def test_multi_equals_solo_and_lock_steps_the_launches(ctx):
    kinds = ["asym", "lambda", "ties", "random", "ints", "tiny"]
    mats = [case(k, n)[:2] for k, n in zip(kinds, MULTI)]
    mj, mf, launches = device_multi(ctx, mats)
    solo_launches = {}
    for (D, V), k, n, gj, gf in zip(mats, kinds, MULTI, mj, mf):
        sj, sf, solo_launches[n] = device_solo(ctx, D, V)
        assert B.same_bits(gj, sj) and B.same_bits(gf, sf), (k, n)
        assert_record(gj, gf, case(k, n)[2], case(k, n)[3], "multi %s n = %d" % (k, n))
    assert launches == solo_launches[257]   # those of the largest family alone
    assert solo_launches[8] % 5 == 0 and solo_launches[257] % 254 == 0
    assert solo_launches[8] // 5 == solo_launches[257] // 254   # a fixed number of kernels per join


def test_rejections(ctx):
    import prographmsa_amd as pg
    INV = pg.PGM_ERR_INVALID
    D, V = case("random", 8)[:2]
    jbuf = np.zeros(8, B.JOIN_DTYPE)
    fbuf = np.zeros(9)
    n8 = np.array([8], np.uint32)
    PJ = jbuf.ctypes.data_as(C.POINTER(pg.pgm_bionj_join))
    PN = n8.ctypes.data_as(C.POINTER(C.c_uint32))
    Dc, Vc = np.ascontiguousarray(D), np.ascontiguousarray(V)
    assert pg.lib.pgm_bionj(None, 8, PD(Dc), PD(Vc), PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj(ctx.handle, 8, None, PD(Vc), PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj(ctx.handle, 8, PD(Dc), None, PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj(ctx.handle, 8, PD(Dc), PD(Vc), None, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj(ctx.handle, 8, PD(Dc), PD(Vc), PJ, None) == INV
    assert pg.lib.pgm_bionj_multi(ctx.handle, 1, None, PD(Dc), PD(Vc), PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj_multi(ctx.handle, 0, PN, PD(Dc), PD(Vc), PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj(ctx.handle, 3, PD(Dc), PD(Vc), PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj(ctx.handle, 32769, PD(Dc), PD(Vc), PJ, PD(fbuf)) == INV   # (refused before anything is read)
    assert pg.lib.pgm_bionj_last_launches(ctx.handle) == 0
    three = (np.ones((3, 3)) - np.eye(3), np.ones((3, 3)) - np.eye(3))
    device_multi(ctx, [(D, V), three, (D, V)], expect=INV)   # n = 3 inside a multi call
    for which in (0, 1):
        for bad in (np.nan, np.inf, -np.inf):
            M = [D.copy(), V.copy()]
            M[which][5, 2] = bad
            device_solo(ctx, M[0], M[1], expect=INV)
            device_multi(ctx, [(D, V), (M[0], M[1])], expect=INV)
    got_j, got_f, launches = device_solo(ctx, D, V)   # a valid call afterwards
    assert_record(got_j, got_f, case("random", 8)[2], case("random", 8)[3], "after the rejections")
    assert launches > 0


# ---- the driver ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


def env_of(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("PGM_DEVICE_BIONJ", "PGM_HOST_BIONJ")}
    env.update(kw)
    return env


def driver(prog, opts, fa, d, tag, env):
    """(stdout, the bytes of the --dump_joins file, --stats) of one run."""
    dj = os.path.join(str(d), tag + ".joins")
    r = bu.run(prog, list(opts) + ["--stats", "--dump_joins", dj, str(fa)], env)
    return r.stdout, open(dj, "rb").read(), bu.stats_of(r.stderr)


def assert_device_equals_oracle(exe, oracle_build, opts, fa, d, host_too=False):
    ref_out, ref_j, ref_st = driver(os.path.join(oracle_build, "pgmsa_oracle"), opts, fa, d, "oracle", env_of())
    assert ref_st["backend"] == "oracle" and ref_st["bionj_device_calls"] == 0 and len(ref_j) > 0 and len(ref_out) > 0
    out, j, st = driver(exe, opts, fa, d, "device", env_of(PGM_DEVICE_BIONJ="1"))
    assert st["backend"] == "hip" and st["bionj_device_calls"] > 0 and st["bionj_launches"] > 0, st
    assert out == ref_out and j == ref_j
    if host_too:
        out, j, st = driver(exe, opts, fa, d, "host", env_of(PGM_HOST_BIONJ="1"))
        assert st["bionj_device_calls"] == 0 and st["bionj_launches"] == 0, st
        assert out == ref_out and j == ref_j


@pytest.mark.parametrize("k", range(len(NW_TREES)), ids=["n%d_s%d" % (c["n"], c["seed"]) for c in NW_TREES])
def test_driver_guide_trees_of_the_golden_families(exe, oracle_build, tmp_path, k):
    c = NW_TREES[k]
    fa = tmp_path / "t.fa"
    fa.write_text(gen.fasta(gen.gen(c["n"], c["L"], c["seed"], sub=c["sub"], indel=c["indel"])))
    assert_device_equals_oracle(exe, oracle_build, ["-T", "-i", "0"], fa, tmp_path, host_too=(k == 0))
    assert_device_equals_oracle(exe, oracle_build, ["-T", "-i", "0", "-a"], fa, tmp_path)


def test_driver_default_flow(exe, oracle_build, tmp_path):
    assert_device_equals_oracle(exe, oracle_build, ["--fasta"], os.path.join(GOLD, "c1.fa"), tmp_path, host_too=True)


def test_driver_wls_refinement(exe, oracle_build, tmp_path):
    c = NW_TREES[-1]
    fa = tmp_path / "t.fa"
    fa.write_text(gen.fasta(gen.gen(c["n"], c["L"], c["seed"], sub=c["sub"], indel=c["indel"])))
    assert_device_equals_oracle(exe, oracle_build, ["-T", "-i", "0", "-W"], fa, tmp_path)


def test_driver_1024_taxa(exe, oracle_build, tmp_path):
    fa = tmp_path / "big.fa"
    fa.write_text(gen.fasta(gen.gen(1024, 300, 11)))
    assert_device_equals_oracle(exe, oracle_build, ["-T", "-i", "0"], fa, tmp_path)


def test_batch_shares_one_call_per_tree_stage(exe, tmp_path):
    """--batch of 12 small families with PGM_DEVICE_BIONJ=1: every output equals the solo run's, and the joins of all families of
    a tree stage are one device call (three stages in the default flow), not one per family."""
    fams = bu.aa_families(tmp_path)
    env = env_of(PGM_DEVICE_BIONJ="1")
    outs, st, _ = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "dev", env=env)
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, ["--fasta"], env=env_of(PGM_HOST_BIONJ="1")))
    assert st["batch_families"] == 12 and st["batch_failed"] == 0
    assert st["bionj_device_calls"] == 3, st
