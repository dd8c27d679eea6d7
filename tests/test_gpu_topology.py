"""--topology on the MI355X: pgm_bionj_plan / pgm_bionj_plan_multi (csrc/pgm_bionj_kernels.h: pgm_bionj_plan_kernel) against the
statement of tests/topology_ref.py bit for bit (tests/test_cpu_topology.py pins that statement to the host loop and to the
goldens), the number of launches, the rejections of the C ABI, and the product driver with PGM_DEVICE_BIONJ=1 against the oracle
driver (host loop): identical stdout and --dump_joins files.  Every driver run is a child process under a time limit of its own."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import batch_util as bu
import bionj_ref as B
import gen
import topology_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GOLDEN = json.load(open(os.path.join(GOLD, "topology.json")))
# one join, both parities of a column's start, the odd last pair, wavefront boundaries, one past the 1024 elements staged in LDS
SIZES = [4, 5, 6, 7, 8, 9, 63, 64, 65, 127, 129, 257, 1025]
KINDS = ["random", "asym", "tiny", "lambda"]
# 16 joins with dim above the 1024 elements (every residue of dim mod 4), for two kinds: the statement takes 2 s more for these eight cases
PAST_CHUNK = [("asym", 1040), ("lambda", 1040)]
GRID = [(kind, n) for kind in KINDS for n in SIZES] + PAST_CHUNK
MULTI = [(4, "asym", "ladder"), (9, "lambda", "random"), (64, "random", "far"), (257, "tiny", "balanced"), (5, "random", "random")]
PD = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


@functools.lru_cache(maxsize=None)
def case(kind, n, plan_kind):
    """(D, V, plan, joins, final_d, info) of one matrix kind, size and plan; the reference is computed once and shared."""
    D, V = B.matrices(kind, n)
    plan = T.plan(plan_kind, n)
    joins, final_d, info = T.bionj_joins_plan(D, V, plan)
    for a in (D, V, joins, final_d):
        a.setflags(write=False)
    return D, V, plan, joins, final_d, info


def plan_array(plans_and_ns):
    """The pairs of the calls' families back to back, n - 3 each (a plan has n - 1)."""
    flat = [p for plan, n in plans_and_ns for p in plan[:n - 3]]
    out = np.zeros((len(flat) + 1, 2), np.uint32)
    out[:len(flat)] = np.array(flat, np.int64).reshape(-1, 2)
    return out


def device_multi(ctx, fams, expect=0):
    """pgm_bionj_plan_multi over [(D, V, plan)]; returns ([joins], [final_d], launches)."""
    import prographmsa_amd as pg
    ns = np.array([D.shape[0] for D, _, _ in fams], np.uint32)
    Dcat = np.ascontiguousarray(np.concatenate([np.asarray(D).reshape(-1) for D, _, _ in fams]))
    Vcat = np.ascontiguousarray(np.concatenate([np.asarray(V).reshape(-1) for _, V, _ in fams]))
    plan = plan_array([(p, int(n)) for (_, _, p), n in zip(fams, ns)])
    joins = np.zeros(int((ns.astype(np.int64) - 3).clip(0).sum()) + 1, B.JOIN_DTYPE)
    final_d = np.full(9 * len(fams), -1.0)
    rc = pg.lib.pgm_bionj_plan_multi(ctx.handle, len(fams), ns.ctypes.data_as(C.POINTER(C.c_uint32)), PD(Dcat), PD(Vcat),
                                     plan.ctypes.data_as(C.POINTER(pg.pgm_bionj_pair)), joins.ctypes.data_as(C.POINTER(pg.pgm_bionj_join)), PD(final_d))
    assert rc == expect, (rc, pg.lib.pgm_last_error())
    out_j, o = [], 0
    for n in ns:
        out_j.append(joins[o:o + max(int(n) - 3, 0)])
        o += max(int(n) - 3, 0)
    return out_j, [final_d[9 * f:9 * f + 9].reshape(3, 3) for f in range(len(fams))], pg.lib.pgm_bionj_last_launches(ctx.handle)


def device_solo(ctx, D, V, plan, expect=0):
    import prographmsa_amd as pg
    n = D.shape[0]
    D, V = np.ascontiguousarray(D), np.ascontiguousarray(V)
    pl = plan_array([(plan, n)])
    joins = np.zeros(max(n - 3, 1), B.JOIN_DTYPE)
    final_d = np.full(9, -1.0)
    rc = pg.lib.pgm_bionj_plan(ctx.handle, n, PD(D), PD(V), pl.ctypes.data_as(C.POINTER(pg.pgm_bionj_pair)),
                               joins.ctypes.data_as(C.POINTER(pg.pgm_bionj_join)), PD(final_d))
    assert rc == expect, (rc, pg.lib.pgm_last_error())
    return joins[:max(n - 3, 0)], final_d.reshape(3, 3), pg.lib.pgm_bionj_last_launches(ctx.handle)


def assert_record(got_j, got_f, ref_j, ref_f, what):
    first = np.flatnonzero((got_j["index1"] != ref_j["index1"]) | (got_j["index2"] != ref_j["index2"]))
    assert first.size == 0, "%s: join %d is %s, the plan has %s" % (what, first[0], got_j[first[0]], ref_j[first[0]])
    assert B.same_bits(got_j, ref_j), "%s: branch lengths differ" % (what,)
    assert B.same_bits(got_f, ref_f), "%s: final_d %s != %s" % (what, got_f, ref_f)


@pytest.mark.parametrize("kind,n", GRID)
def test_plan_kernel_matches_the_statement(ctx, kind, n):
    for plan_kind in T.PLANS:
        D, V, plan, ref_j, ref_f, _ = case(kind, n, plan_kind)
        assert T.read_plan_joins(ref_j) == plan[:n - 3]
        if plan_kind == "ladder":
            assert all(p == (0, 1) for p in plan)
        if plan_kind == "far":
            assert all(p == (n - 2 - s, n - 1 - s) for s, p in enumerate(plan))   # index2 = dim - 1
        D0, V0 = D.copy(), V.copy()
        got_j, got_f, launches = device_solo(ctx, D, V, plan)
        assert B.same_bits(D, D0) and B.same_bits(V, V0)   # the inputs are not modified
        assert_record(got_j, got_f, ref_j, ref_f, "%s %s n = %d" % (kind, plan_kind, n))
        assert 0 < launches <= 3
    if kind == "tiny":
        D, V = case(kind, n, "ladder")[:2]
        assert (D[D > 0] < B.MIN_DIST).any() and (V[V > 0] < B.MIN_VAR).any()


def test_lambda_cases_take_both_clamps():
    """The V rows of `lambda` are scaled by 100 or by 1, so a join of a scaled with an unscaled row drives lambda out of [0, 1],
    on the side that depends on which of the two has the smaller index: over the four plans of a size both sides occur."""
    total = dict(lambda_at_0=0, lambda_at_1=0)
    for n in SIZES:
        infos = [case("lambda", n, p)[5] for p in T.PLANS]
        for key in total:
            here = sum(i[key] for i in infos)
            total[key] += here
            assert n < 7 or here > 0, (n, key, infos)
    assert total["lambda_at_0"] > 0 and total["lambda_at_1"] > 0


def test_multi_equals_solo(ctx):
    """Mixed sizes in one call: a family that is done long before the others."""
    fams = [case(kind, n, p)[:3] for n, kind, p in MULTI]
    mj, mf, launches = device_multi(ctx, fams)
    for (D, V, plan), (n, kind, p), gj, gf in zip(fams, MULTI, mj, mf):
        sj, sf, solo_launches = device_solo(ctx, D, V, plan)
        assert B.same_bits(gj, sj) and B.same_bits(gf, sf), (kind, n)
        assert_record(gj, gf, case(kind, n, p)[3], case(kind, n, p)[4], "multi %s %s n = %d" % (kind, p, n))
        assert launches == solo_launches


def test_the_number_of_launches_does_not_depend_on_n(ctx):
    l8 = device_solo(ctx, *case("random", 8, "random")[:3])[2]
    l257 = device_solo(ctx, *case("random", 257, "random")[:3])[2]
    assert l8 == l257 and 0 < l8 <= 3


def test_rejections(ctx):
    import prographmsa_amd as pg
    INV = pg.PGM_ERR_INVALID
    launches = lambda: pg.lib.pgm_bionj_last_launches(ctx.handle)
    D, V, plan, ref_j, ref_f, _ = case("random", 8, "random")
    Dc, Vc = np.ascontiguousarray(D), np.ascontiguousarray(V)
    pl = plan_array([(plan, 8)])
    PP = pl.ctypes.data_as(C.POINTER(pg.pgm_bionj_pair))
    jbuf = np.zeros(8, B.JOIN_DTYPE)
    fbuf = np.zeros(9)
    PJ = jbuf.ctypes.data_as(C.POINTER(pg.pgm_bionj_join))
    n8 = np.array([8], np.uint32)
    PN = n8.ctypes.data_as(C.POINTER(C.c_uint32))
    assert pg.lib.pgm_bionj_plan(None, 8, PD(Dc), PD(Vc), PP, PJ, PD(fbuf)) == INV
    for args in [(None, PD(Vc), PP, PJ, PD(fbuf)), (PD(Dc), None, PP, PJ, PD(fbuf)), (PD(Dc), PD(Vc), None, PJ, PD(fbuf)),
                 (PD(Dc), PD(Vc), PP, None, PD(fbuf)), (PD(Dc), PD(Vc), PP, PJ, None)]:
        assert pg.lib.pgm_bionj_plan(ctx.handle, 8, *args) == INV and launches() == 0
    assert pg.lib.pgm_bionj_plan_multi(ctx.handle, 1, None, PD(Dc), PD(Vc), PP, PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj_plan_multi(ctx.handle, 0, PN, PD(Dc), PD(Vc), PP, PJ, PD(fbuf)) == INV
    assert pg.lib.pgm_bionj_plan(ctx.handle, 3, PD(Dc), PD(Vc), PP, PJ, PD(fbuf)) == INV and launches() == 0   # n < 4
    assert pg.lib.pgm_bionj_plan(ctx.handle, 32769, PD(Dc), PD(Vc), PP, PJ, PD(fbuf)) == INV   # (refused before anything is read)
    three = (np.ones((3, 3)) - np.eye(3), np.ones((3, 3)) - np.eye(3), [])
    device_multi(ctx, [(D, V, plan), three, (D, V, plan)], expect=INV)   # n = 3 inside a multi call
    assert launches() == 0
    # plan entries: index1 == index2, index1 > index2, index2 == dim at the first join, at a later join, far out of range
    for step, pair in [(0, (2, 2)), (1, (3, 1)), (0, (0, 8)), (3, (1, 5)), (4, (0, 4)), (2, (0, 0xFFFFFFFF))]:
        bad = list(plan)
        bad[step] = pair
        device_solo(ctx, D, V, bad, expect=INV)
        assert launches() == 0
        device_multi(ctx, [(D, V, plan), (D, V, bad)], expect=INV)
        assert launches() == 0
    ok = list(plan)
    ok[4] = (0, 3)   # (the last index the fifth join of eight taxa may name)
    device_solo(ctx, D, V, ok)
    for which in (0, 1):
        for bad in (np.nan, np.inf, -np.inf):
            M = [D.copy(), V.copy()]
            M[which][5, 2] = bad
            device_solo(ctx, M[0], M[1], plan, expect=INV)
            assert launches() == 0
            device_multi(ctx, [(D, V, plan), (M[0], M[1], plan)], expect=INV)
            assert launches() == 0
    got_j, got_f, n_launch = device_solo(ctx, D, V, plan)   # a valid call afterwards
    assert_record(got_j, got_f, ref_j, ref_f, "after the rejections")
    assert n_launch > 0


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


def assert_device_equals_oracle(exe, oracle_build, opts, fa, d, trees=1, host_too=False):
    ref_out, ref_j, ref_st = driver(os.path.join(oracle_build, "pgmsa_oracle"), opts, fa, d, "oracle", env_of())
    assert ref_st["backend"] == "oracle" and ref_st["bionj_device_calls"] == 0 and len(ref_j) > 0 and len(ref_out) > 0
    out, j, st = driver(exe, opts, fa, d, "device", env_of(PGM_DEVICE_BIONJ="1"))
    assert st["backend"] == "hip" and st["bionj_device_calls"] == trees and 0 < st["bionj_launches"] <= 3 * trees, st
    assert out == ref_out and j == ref_j
    if host_too:   # the default: the host loop
        out, j, st = driver(exe, opts, fa, d, "host", env_of())
        assert st["bionj_device_calls"] == 0 and st["bionj_launches"] == 0, st
        assert out == ref_out and j == ref_j
    return ref_out


@pytest.mark.parametrize("k", [0, 5, 11], ids=["n5", "n11", "n30"])
def test_driver_on_golden_families(exe, oracle_build, tmp_path, k):
    fam = sorted(set((c["n"], c["L"], c["seed"], c["sub"], c["indel"]) for c in GOLDEN["trees"]))[k]
    n, L, seed, sub, indel = fam
    fa = tmp_path / "t.fa"
    fa.write_text(gen.fasta(gen.gen(n, L, seed, sub=sub, indel=indel)))
    for c in GOLDEN["trees"]:
        if (c["n"], c["L"], c["seed"], c["sub"], c["indel"]) == fam and c["flow"] == "nw" and c["kind"] in ("swapped", "extra_leaves"):
            tp = tmp_path / (c["kind"] + ".nwk")
            tp.write_text(c["topology"] + "\n")
            out = assert_device_equals_oracle(exe, oracle_build, ["-a", "-T", "-i", "0", "--topology", str(tp)], fa, tmp_path, host_too=(c["kind"] == "swapped"))
            assert out == c["stdout"]


def test_driver_300_taxa(exe, oracle_build, tmp_path):
    fa = tmp_path / "big.fa"
    fa.write_text(gen.fasta(gen.gen(300, 60, 11)))
    tp = tmp_path / "big.nwk"
    tp.write_text(T.format_topology(T.random_tree(["seq%04d" % i for i in range(300)], random.Random(300))) + "\n")
    assert_device_equals_oracle(exe, oracle_build, ["-a", "-T", "-i", "0", "--topology", str(tp)], fa, tmp_path)


def test_driver_default_flow(exe, oracle_build, tmp_path):
    """Every re-estimation keeps the topology: one device call per tree."""
    c = GOLDEN["fasta"][0]
    tp = tmp_path / "t.nwk"
    tp.write_text(c["topology"] + "\n")
    ref_out, ref_j, _ = driver(os.path.join(oracle_build, "pgmsa_oracle"), ["--fasta", "--topology", str(tp)], os.path.join(GOLD, c["fasta"]), tmp_path, "oracle", env_of())
    out, j, st = driver(exe, ["--fasta", "--topology", str(tp)], os.path.join(GOLD, c["fasta"]), tmp_path, "device", env_of(PGM_DEVICE_BIONJ="1"))
    assert out == ref_out == c["stdout"] and j == ref_j
    assert 2 <= st["bionj_device_calls"] <= 3 and st["bionj_launches"] <= 3 * st["bionj_device_calls"], st


def test_batch_with_fourth_fields(exe, oracle_build, tmp_path):
    """A mixed list under PGM_DEVICE_BIONJ=1: the families with a topology are one bionj_plan_multi call, the plain ones one
    bionj_multi call, and every output is the oracle driver's solo output."""
    fams = T.topology_families(tmp_path)
    opts = ["-a", "-T", "-i", "0"]
    st = T.batch_against_solo(exe, os.path.join(oracle_build, "pgmsa_oracle"), fams, opts, tmp_path, env=env_of(PGM_DEVICE_BIONJ="1"), solo_env=env_of())
    assert st["backend"] == "hip" and st["batch_families"] == len(fams) and st["batch_failed"] == 0
    plain = [n for n in (len(open(fa).read().split(">")) - 1 for fa, tree, topo in fams if not tree and not topo) if n >= 4]
    assert st["bionj_device_calls"] == 2, st
    assert st["bionj_launches"] <= 3 + 3 * (max(plain) - 3), st
