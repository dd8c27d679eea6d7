"""`--ml_spr` through the CPU oracle driver (pgmsa_oracle: Backend::tree_spr's default, the host loop), and the pieces below it:
  - tests/treelik_spr_ref.py itself against brute force (every candidate's regrafted tree built and evaluated by treelik_rates_ref);
  - tree_spr_host in a stand-alone program (tests/native/treelik_spr_test.cpp), its %a output equal to the statement bit for bit, and
    the moves of the scan applied to trees; built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, runs without the flag, the log with the flag, a simulated family whose start is one SPR away."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import mldist_general_ref as M
import test_cpu_mlsearch as TS
import test_cpu_mlsupport as TSUP
import test_cpu_mltree as TM
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
import treelik_spr_ref as S
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Ten times the largest relative difference measured between the statement and the brute-force ratio over every case below
# (1.6e-15), as DESIGN 3.20 and 3.22 set theirs; anything above 1e-10 would be a defect, not a tolerance.
BRUTE_BOUND = 1.6e-14
# The same for the caterpillar's scaling cases, compared in log space: measured 6.33e-14 (log rho is a difference of two
# log-likelihoods near 600 in size, so their rounding is in it), the test asserts ten times that.
CATERPILLAR_BOUND = 6.33e-13
assert BRUTE_BOUND <= 1e-10 and CATERPILLAR_BOUND <= 1e-10


# ---- the statement against brute force ---------------------------------------------------------------------------------------------------
def generator_case(dim, tree, ncat, seed):
    """A case whose matrices are exp(Q r t) and exp(Q r t / 2) of a seeded generator that is not reversible; columns with gaps and
    -2; every valid candidate of the tree."""
    nleaves, parent = S.TREES[tree]()
    nedges = len(parent) - 1
    rng = np.random.default_rng(seed)
    Q = M.random_generator(dim, 40 + dim)
    pi = rng.dirichlet(np.ones(dim) * 3)
    lengths = rng.uniform(0.05, 0.6, nedges)
    rates, w = (np.array([1.0]), np.array([1.0])) if ncat == 1 else (np.array([0.2, 0.7, 1.1, 2.0]), np.full(4, 0.25))
    ncols = 7
    rows = rng.integers(0, dim, (nleaves, ncols)).astype(np.int8)
    rows[0, 1] = -1; rows[:, 2] = -1; rows[nleaves - 1, 3] = -2; rows[1, 4] = -2; rows[2, 4] = -1
    P = G.matrices(Q, lengths, rates, derivs=False)
    Ph = G.matrices(Q, lengths / 2, rates, derivs=False)
    cand = S.candidates(nleaves, parent)
    return dict(dim=dim, nleaves=nleaves, parent=parent, rows=rows, pi=pi, w=w, P=P, Ph=Ph, tree=tree, ncat=ncat, cand=cand,
                want=S.evaluate(dim, nleaves, parent, rows, pi, w, P, Ph, cand))


BRUTE = [(dim, tree, ncat) for dim in (4, 20) for tree in ("balanced8", "trifurcating", "inner3") for ncat in (1, 4)]


@pytest.mark.parametrize("dim,tree,ncat", BRUTE)
def test_reference_against_brute_force(dim, tree, ncat):
    """Every valid candidate of the balanced tree of 8, of the trifurcating root and of the tree with an inner trifurcation (y = p and
    y a sibling of v among them), under a generator that is not reversible: rho against sum_k w_k L'_k / sum_k w_k L_k of the
    regrafted tree, a dissolved p as the matrix product P_p P_s, the new node with Ph_y twice, the tree renumbered."""
    case = generator_case(dim, tree, ncat, 900 + dim + ncat + sum(map(ord, tree)))
    want, parent, nleaves = case["want"], case["parent"], case["nleaves"]
    assert np.array_equal(case["cand"], S.candidates_by_path(nleaves, parent))
    if tree == "inner3":   # node 6 = (0, 1, 2): a prune node whose parent keeps two children takes y = p and y a sibling
        pairs = [tuple(x) for x in case["cand"].tolist()]
        assert (0, 6) in pairs and (0, 1) in pairs and (0, 2) in pairs
    if tree == "balanced8":   # p of two children: neither y = p nor the sibling, and no prune node below a binary root
        pairs = [tuple(x) for x in case["cand"].tolist()]
        assert (0, 8) not in pairs and (0, 1) not in pairs and not any(v in (10, 13) for v, _ in pairs) and len(pairs) == 124
    own = G.evaluate(dim, nleaves, parent, case["rows"], case["pi"], case["w"], case["P"], derivs=False)
    worst = 0.0
    for q, (v, y) in enumerate(case["cand"]):
        log_ratio = S.brute_log_rho(dim, nleaves, parent, case["rows"], case["pi"], case["w"], case["P"], case["Ph"], int(v), int(y), own)
        ratio = np.exp(log_ratio)
        assert np.all(np.isfinite(ratio)) and np.all(ratio > 0)
        parent2, spec = S.regrafted(nleaves, parent, int(v), int(y))
        there = G.evaluate(dim, nleaves, parent2, case["rows"], case["pi"], case["w"],
                           S.regrafted_matrices(dim, ncat, len(parent) - 1, case["P"], case["Ph"], spec), derivs=False)
        assert np.all(there["site_k"] == 0) and np.all(own["site_k"] == 0)
        exact = there["site_l"] / own["site_l"]
        worst = max(worst, float(np.max(np.abs(want["rho"][q] - exact) / exact)))
    print("largest relative difference: %.3g" % worst)
    assert worst < BRUTE_BOUND


def test_caterpillar_scaling_in_log_space():
    """The caterpillar of 96 leaves, every matrix entry in [0.03, 0.07]: paths of up to 16 edges, every rho finite and above 0, some
    candidate has k- != k+ on some column, and log rho is within CATERPILLAR_BOUND of the brute-force log ratio."""
    case = caterpillar_case(4, 1)
    want = case["want"]
    assert np.all(np.isfinite(want["rho"])) and np.all(want["rho"] > 0)
    lens = [len(p[0]) - 1 + len(p[1]) for p in (S.path_of(case["parent"], int(v), int(y)) for v, y in case["cand"])]
    assert {1, 2, 15, 16} <= set(lens) and max(lens) == 16
    differs = np.argwhere((want["cat_km"][0] != want["cat_kp"][0]).any(axis=1))[:, 0]
    assert len(differs) > 0
    own = G.evaluate(4, case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], derivs=False)
    worst = 0.0
    for q in sorted(set(list(differs[:5]) + list(differs[-5:]) + [int(np.argmax(lens))])):
        v, y = (int(x) for x in case["cand"][q])
        log_ratio = S.brute_log_rho(4, case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["Ph"], v, y, own)
        worst = max(worst, float(np.max(np.abs(np.log(want["rho"][q]) - log_ratio))))
    print("largest difference of log rho: %.3g" % worst)
    assert worst < CATERPILLAR_BOUND


def test_zero_denominator_gives_zero():
    """Matrices that hold zeros: category 0 is the identity on every edge, so a column whose leaves differ has D == 0 there and the
    category's ratio is 0.0, not 0 / 0; the mixture stays finite and is the other category's term."""
    case = zeros_case()
    want = case["want"]
    hit = want["cat_l"][0] == 0.0   # the columns whose states cannot all be one state
    assert hit.any() and not hit.all()
    assert np.all(want["cat_rho"][0][:, hit] == 0.0) and np.all(want["post"][0][hit] == 0.0)
    assert np.all(np.isfinite(want["rho"])) and np.all(want["rho"][:, hit] > 0)


# ---- the cases of the host loop and of tests/test_gpu_mlspr.py, which takes these lists from here ---------------------------------------
DIMS = (4, 20, 61, 64)
GRID = [(dim, ncols, "balanced8", ncat) for dim in DIMS for ncols in (1, 15, 16, 17, 33) for ncat in (1, 2, 4)]
ODD_DIMS = [(dim, ncols, "balanced8", 2) for dim in (1, 2, 3, 5, 33, 63) for ncols in sorted({1, 64 // dim, 64 // dim + 1, 4 * (64 // dim) + 1})]
TREES = ([(dim, 17, "three", 2) for dim in DIMS] + [(dim, 17, "four", 2) for dim in DIMS]
         + [(dim, 17, tree, 2) for dim in (4, 20) for tree in ("trifurcating", "mixed3", "inner3")] + [(20, 33, "balanced24", 4, "all", 3)])
WIDE = [(4, 1025, "balanced8", 2)]
ORDER = [(4, 33, "balanced8", 4, "one"), (20, 17, "balanced8", 2, "shuffled"), (4, 33, "inner3", 4, "shuffled")]
SMALL_VALID = (4, 15, "balanced8", 2)   # what the rejections change
MADE = list(dict.fromkeys(GRID + ODD_DIMS + TREES + WIDE + ORDER + [SMALL_VALID]))


def caterpillar_list():
    """Candidates of the caterpillar of 96 whose paths have 1, 2, 15 and 16 edges, upward and across the turn: those of every twelfth
    prune node, which takes in the depths where the two chains of a candidate cross the scaling threshold at different steps."""
    _, parent = S.TREES["caterpillar96"]()
    cand = S.candidates(96, parent, 16)
    lens = np.array([len(p[0]) - 1 + len(p[1]) for p in (S.path_of(parent, int(v), int(y)) for v, y in cand)])
    return cand[np.isin(lens, (1, 2, 15, 16)) & (cand[:, 0] % 12 == 0)]


def caterpillar_case(dim, ncat):
    return S.make_case(dim, 17, "caterpillar96", ncat, caterpillar_list())


def leaf_case():
    """Leaves with a state, a gap or -2 as v and as y, and columns of gaps alone: (((0,1)4,2)5,3)6 with hand-made rows."""
    base = S.make_case(4, 15, "four", 2, "one")
    parent = np.array([4, 4, 5, 6, 5, 6, R.ROOT], np.uint32)
    rows = np.array([[0, -1, -2, 1, -1, 2, 3, -1],
                     [1, 2, 3, -1, -1, -2, 0, -1],
                     [2, 2, -1, -2, -1, 0, 1, -1],
                     [3, -2, 0, 2, -1, -1, -2, -1]], np.int8)
    cand = S.candidates(4, parent)
    assert {0, 1, 2} <= set(cand[:, 0].tolist()) and {0, 2, 3} <= set(cand[:, 1].tolist())   # (leaves as v and as y)
    return dict(dim=4, nleaves=4, parent=parent, rows=rows, pi=base["pi"], w=base["w"], P=base["P"], Ph=base["Ph"], tree="leaves", ncat=2, cand=cand,
                want=S.evaluate(4, 4, parent, rows, base["pi"], base["w"], base["P"], base["Ph"], cand))


def zeros_case():
    base = S.make_case(4, 15, "balanced8", 2)
    nedges = len(base["parent"]) - 1
    eye = R.pack(np.tile(np.eye(4), (nedges, 1, 1, 1)))
    P, Ph = base["P"].copy(), base["Ph"].copy()
    P[:len(eye)] = eye
    Ph[:len(eye)] = eye
    rows = base["rows"].copy()
    rows[:, 0] = 2; rows[:, 9] = 1   # columns whose leaves agree: the identity keeps them
    cand = base["cand"][::7]
    return dict(base, P=P, Ph=Ph, rows=rows, cand=cand, tree="balanced8, zeros", want=S.evaluate(4, 8, base["parent"], rows, base["pi"], base["w"], P, Ph, cand))


def many_candidates_case():
    """More candidates than a grid's second dimension holds (65535): the caterpillar's list, 70001 in turn, dim 2, one column.  The
    expectation is that of the list, repeated."""
    base = S.make_case(2, 1, "caterpillar96", 2, caterpillar_list())
    pick = np.arange(70001) % len(base["cand"])
    want = dict(base["want"])
    want["rho"] = np.ascontiguousarray(base["want"]["rho"][pick])
    return dict(base, cand=np.ascontiguousarray(base["cand"][pick]), want=want, tree="caterpillar96, 70001 candidates")


def all_cases():
    return [S.make_case(*k) for k in MADE] + [caterpillar_case(4, 1), caterpillar_case(20, 2), leaf_case(), zeros_case(), many_candidates_case()]


def bad_candidates():
    """What the entry refuses among the candidates of the balanced tree of 8 (8 = (0, 1), 9 = (2, 3), 10 = (8, 9), 11 = (4, 5),
    12 = (6, 7), 13 = (11, 12), the root 14 = (10, 13)): v or y the root or beyond the nodes; y in the subtree of v or v itself; the
    parent of v a root of two children; y the parent or the sibling of a v whose parent has two children; one of these behind a valid one."""
    return [[[14, 0]], [[15, 0]], [[0xFFFFFFFF, 0]], [[0, 14]], [[0, 15]], [[0, 0xFFFFFFFF]], [[10, 0]], [[10, 10]], [[8, 8]], [[3, 3]], [[10, 4]], [[13, 0]],
            [[0, 8]], [[0, 1]], [[8, 10]], [[8, 9]], [[0, 9], [0, 1]]]


def long_path_case(extra):
    """The caterpillar of 96: leaf 1 onto the edge above an inner node 16 + extra edges up the spine (extra == 0: the longest the
    entry takes)."""
    base = S.make_case(2, 1, "caterpillar96", 2, caterpillar_list())
    parent = base["parent"]
    v, y = 1, int(parent[1])
    for _ in range(S.MAXPATH + extra):
        y = int(parent[y])
    return dict(base, cand=np.array([[v, y]], np.uint32)), (v, y)


def _case_bytes(c, **kw):
    d = dict(c); d.update(kw)
    nnodes = d.get("nnodes", len(d["parent"]))
    cand = np.asarray(d["cand"], np.uint32).reshape(-1, 2)
    head = np.array([d["dim"], d["nleaves"], nnodes, d["rows"].shape[1], d["ncat"], d.get("ncand", len(cand))], np.int32)
    parts = [head, np.asarray(d["parent"], np.uint32), np.asarray(d["rows"], np.int8), np.asarray(d["pi"], np.float64), np.asarray(d["w"], np.float64),
             np.asarray(d["P"], np.float64), np.asarray(d["Ph"], np.float64), cand]
    return b"".join(np.ascontiguousarray(x).tobytes() for x in parts)


def _bad_cases():
    c = S.make_case(*SMALL_VALID)
    bad = [_case_bytes(c, cand=np.zeros((0, 2), np.uint32))]   # no candidate
    for cand in bad_candidates():
        bad.append(_case_bytes(c, cand=np.array(cand, np.uint32)))
    bad.append(_case_bytes(long_path_case(1)[0]))   # 17 edges
    nspr = len(bad)
    for ncat in (0, 17):
        bad.append(_case_bytes(c, ncat=ncat, w=np.full(ncat, 0.5), P=np.tile(c["P"][:len(c["P"]) // 2], ncat), Ph=np.tile(c["Ph"][:len(c["Ph"]) // 2], ncat)))
    for v in (0.0, float("nan")):
        bad.append(_case_bytes(c, w=np.array([0.5, v])))
    for b in TM._bad_cases():
        bad.append(_case_bytes(c, parent=b["parent"], rows=b["rows"], cand=c["cand"][:1]))
    return bad, nspr


def test_the_longest_path_is_taken():
    case, (v, y) = long_path_case(0)
    up, down = S.path_of(case["parent"], v, y)
    assert len(up) - 1 + len(down) == 16
    up, down = S.path_of(long_path_case(1)[0]["parent"], *long_path_case(1)[1])
    assert len(up) - 1 + len(down) == 17


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("spr_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_spr_test.cpp"), os.path.join(host, "treelik_spr.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    cases = all_cases() + [long_path_case(0)[0]]
    cases[-1] = dict(cases[-1], want=S.evaluate(2, 96, cases[-1]["parent"], cases[-1]["rows"], cases[-1]["pi"], cases[-1]["w"], cases[-1]["P"], cases[-1]["Ph"], cases[-1]["cand"]))
    bad, nspr = _bad_cases()
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases) + len(bad)], np.int32).tobytes())
        for c in cases:
            f.write(_case_bytes(c))
        for blob in bad:
            f.write(blob)
    # (-fno-sanitize=vptr: as tests/test_cpu_mltree.py, the unit holds Backend's virtual defaults without the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("spr_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    for name in flags:
        r = subprocess.run([str(d / ("spr_test_" + name)), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % (len(cases) + len(bad))), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    # the plain build again, holding the pieces of one column chunk at a time: every case of 17 and of 33 columns takes 2 and 3 blocks
    r = subprocess.run([str(d / "spr_test_plain"), path, "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0
    out["plain, a block per chunk"] = r.stdout.splitlines()
    return SimpleNamespace(cases=cases, bad=bad, nspr=nspr, lines=out, exes={name: str(d / ("spr_test_" + name)) for name in flags})


@pytest.mark.parametrize("build", ["plain", "sanitized", "plain, a block per chunk"])
def test_host_loop_equals_the_statement(native, build):
    lines, cases = native.lines[build], native.cases
    floats = lambda text: np.array([float.fromhex(x) for x in text.split()])
    for k, c in enumerate(cases):
        l, kk, post, rho, gain = lines[5 * k:5 * k + 5]
        want, what = c["want"], (build, k, c["dim"], c["tree"], c["ncat"])
        assert not np.any(np.isnan(want["rho"])), what
        assert R.same_bits(floats(l), want["site_l"]), what
        assert np.array_equal(np.array([int(x) for x in kk.split()], np.int32), want["site_k"]), what
        assert R.same_bits(floats(post).reshape(want["post"].shape), want["post"]), what
        assert R.same_bits(floats(rho).reshape(want["rho"].shape), want["rho"]), what
        if len(c["cand"]) < 1000:
            assert R.same_bits(floats(gain), N.gain(want["rho"])), what
    assert any(len(c["cand"]) == 70001 for c in cases)
    first = 5 * len(cases)
    rejected = lines[first:first + len(native.bad)]
    assert len(rejected) == len(native.bad) and all(line.startswith("rejected tree ") for line in rejected), rejected   # (no "(outputs written)")
    assert sum(line.startswith("rejected tree spr:") for line in rejected) == native.nspr
    assert any("more than 16 edges" in line for line in rejected)
    assert len(lines) == first + len(native.bad) + 1


def test_statement_properties():
    """site_l, site_k and post are the rates entry's; a column of gaps gives 1 within rounding; the order of the candidates and their
    repeats change no bit of a row."""
    for key in [(4, 33, "balanced8", 4), (20, 17, "balanced8", 2, "shuffled"), (20, 17, "trifurcating", 2)]:
        c = S.make_case(*key)
        old = G.evaluate(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"], derivs=False)
        for k in ("site_l", "site_k", "post"):
            assert R.same_bits(c["want"][k], old[k]), (key, k)
        assert np.max(np.abs(c["want"]["rho"][:, 3] - 1)) < 1e-12   # (site 3 is all gaps; the matrices are row-stochastic)
    c = S.make_case(20, 17, "balanced8", 2, "shuffled")
    full = S.make_case(20, 17, "balanced8", 2)
    for q, cand in enumerate(c["cand"]):
        at = [tuple(x) for x in full["cand"].tolist()].index(tuple(cand.tolist()))
        assert R.same_bits(c["want"]["rho"][q], full["want"]["rho"][at])
    w = leaf_case()["want"]
    assert np.max(np.abs(w["rho"][:, 4] - 1)) < 1e-12 and np.max(np.abs(w["rho"][:, 7] - 1)) < 1e-12
    assert np.all(np.isfinite(w["rho"])) and np.all(w["rho"] > 0)
    three = S.make_case(4, 17, "three", 2)
    assert three["cand"].tolist() == [[0, 2], [1, 2]]   # ((0, 1), 2): one target, and it lies beyond the root (J == 1, M == 1)


MOVE_TREES = [TS.TRUE8, TS.TRUE6, "((a:0.1,b:0.2,c:0.3):0.1,(d:0.1,e:0.2):0.3,(f:0.1,(g:0.2,h:0.1):0.2,i:0.05):0.2);",
              "((((((((((a:1,b:1):1,c:1):1,d:1):1,e:1):1,f:1):1,g:1):1,h:1):1,i:1):1,j:1):1,k:1);"]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_picked_moves_give_trees(native, build):
    """Greedy sets of moves with disjoint touched sets, in 40 seeded orders per tree and radius, applied together: ml_tree_topology takes
    every resulting tree, the leaves are the same, the lengths stay in their interval."""
    for text in MOVE_TREES:
        for radius in (1, 3, 10):
            r = subprocess.run([native.exes[build], "moves", str(radius), text], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stdout.startswith("moves ok "), (text, radius, r.stdout, r.stderr[-2000:])
            names, parent, _ = R.from_newick(text)
            assert int(r.stdout.split()[2]) == len(S.candidates(len(names), parent, radius)), (text, radius)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


# The generating tree of the simulated families is test_cpu_mlsearch's TRUE8.  The start has t1 beside (t5, t6): the generating tree is
# one SPR of 4 edges away (t1 pruned from beside (t5, t6), regrafted on the edge above t2; up 2, down 2), through the root.  600
# columns, seed 4 of the simulator below: the interchanges alone stop two splits short (lnL -4558.0), the scan finds the move
# (lnL -4534.9).  Found on the CPU with pgmsa_oracle among seeds 1 .. 8 at 300 and 600 columns.
TRUE8 = TS.TRUE8
SPR_START = "((t2:0.15,(t3:0.2,t4:0.1):0.2):0.15,(((t5:0.12,t6:0.18):0.12,t1:0.1):0.12,(t7:0.1,t8:0.2):0.3):0.1);"
SPR_SEED, SPR_COLS = 4, 600
simulate_dna = TS.simulate_dna   # (the simulator of tests/test_cpu_mlsearch.py: seeded numpy, no indels)


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("spr_fams")
    aa = bu.aa_families(d)
    out = dict(aa5=[f for f in aa if f.endswith("_n5.fa")][0], aa8=[f for f in aa if f.endswith("_n8.fa")][0], hky=bu.hky_model(d), dir=d)
    hky = R.custom(out["hky"], 4)
    out["sim8"] = os.path.join(str(d), "sim8.fa")
    simulate_dna(out["sim8"], hky, TRUE8, TS.SEED8, 2000)
    out["spr8"] = os.path.join(str(d), "spr8.fa")
    simulate_dna(out["spr8"], hky, TRUE8, SPR_SEED, SPR_COLS)
    for name, text in [(k, v[0]) for k, v in TS.STARTS.items()] + [("true", TRUE8), ("spr_start", SPR_START)]:
        out[name] = TS.write(os.path.join(str(d), name + ".nwk"), text)
    return out


DNA = TS.DNA


def test_refusals(exe, fams, tmp_path):
    fa = fams["aa5"]
    tree, log = str(tmp_path / "never.tree"), str(tmp_path / "never.log")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    ml, se = ["--ml_tree", tree], ["--ml_search", "3", "--ml_search_log", log]
    cases = [
        (["--ml_spr", "3", fa], "--ml_spr needs --ml_tree"),
        (ml + ["--ml_spr", "3", fa], "--ml_spr needs --ml_search"),
        (ml + ["--ml_spr", "3", "--ml_start", fams["true"], fa], "--ml_spr needs --ml_search"),
        (ml + se + ["--ml_spr", "3", "-W", fa], "cannot be combined with -W"),
        (ml + se + ["--ml_spr", "3", "--batch", lst], "--batch cannot be combined"),
    ]
    for text in ("0", "11", "-1", "abc", "1.5", "", "3x"):
        cases.append((ml + se + ["--ml_spr", text, fa], "--ml_spr takes a radius from 1 to 10"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta", "-i", "0"] + args, code=2)
        assert "ERROR:" in r.stderr and message in r.stderr, (args, r.stderr)
        assert r.stdout == "" and not any(os.path.exists(p) for p in (tree, log)), args
    h = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "ml_spr" not in h.stdout + h.stderr


def hangs_together(log, eps=TS.EPSILON):
    """Every line: lnl_before <= lnl_applied <= lnl_after, a line that applied nothing carries its lnL through, a round starts where the
    line before it ended, and lnL never falls."""
    last = None
    for line in log:
        applied, before, there, after = int(line[3]), float(line[5]), float(line[6]), float(line[7])
        assert before <= there <= after, line
        if applied == 0:
            assert before == there == after, line
        else:
            assert there > before and float(line[4]) > eps and int(line[2]) >= applied, line
        if last is not None:
            assert before == last, line
        last = after
    return last


@pytest.fixture(scope="module")
def runs(exe, fams, tmp_path_factory):
    """The simulated family from its SPR start, and sim8 from the start whose interchanges pass through the third resolution: without
    the flag and with it."""
    d = tmp_path_factory.mktemp("spr_runs")
    out = {}
    for fam, start in (("spr8", "spr_start"), ("sim8", "swapped_pairs")):
        out[fam, None] = TS.run_s(exe, fams[fam], d, fam + "_plain", DNA(fams), search=20, start=fams[start])
        for radius in (2, 4):
            out[fam, radius] = TS.run_s(exe, fams[fam], d, "%s_r%d" % (fam, radius), DNA(fams) + ["--ml_spr", str(radius)], search=20, start=fams[start])
    return out


def test_without_the_flag_nothing_changes(runs):
    for fam in ("spr8", "sim8"):
        plain = runs[fam, None]
        assert not any(k.startswith("ml_spr") for k in plain.stats) and all(len(line) == 8 for line in plain.log)
        assert int(plain.log[-1][3]) == 0 and len(plain.log) == plain.stats["ml_search_rounds"] + 1   # (it ends on a round that applied nothing)


@pytest.mark.parametrize("fam", ["spr8", "sim8"])
@pytest.mark.parametrize("radius", [2, 4])
def test_log_with_the_flag(runs, fam, radius):
    """Up to the first spr line the log is the run's without the flag (a ninth column aside); ml_lnl is never lower; every log hangs
    together; where a scan applied one move, lnl_applied - lnl_before is the move's gain, which ties rho to a full evaluation."""
    plain, run = runs[fam, None], runs[fam, radius]
    assert all(len(line) == 9 and line[8] in ("nni", "spr") for line in run.log)
    kinds = [line[8] for line in run.log]
    assert "spr" in kinds
    first = kinds.index("spr")
    assert [line[:8] for line in run.log[:first]] == plain.log and all(k == "nni" for k in kinds[:first])
    assert run.stats["ml_lnl"] >= plain.stats["ml_lnl"]
    assert hangs_together(run.log) == run.stats["ml_lnl"] and hangs_together(plain.log) == plain.stats["ml_lnl"]
    assert run.log[-1][8] == "spr" and int(run.log[-1][3]) == 0 and int(run.log[-2][3]) == 0   # it ends where neither step applies a move
    scans = [line for line in run.log if line[8] == "spr"]
    for line in scans:
        assert int(line[1]) > 0
        if int(line[3]) == 1:
            assert abs((float(line[6]) - float(line[5])) - float(line[4])) <= 1e-9 * abs(float(line[5])), line
    s = run.stats
    assert s["ml_spr_calls"] == len(scans) and s["ml_spr_candidates"] == sum(int(line[1]) for line in scans)
    assert s["ml_spr_applied"] == sum(int(line[3]) for line in scans) and s["ml_spr_s"] > 0 and s["ml_spr_kernel_ms"] == 0
    assert s["ml_nni_applied"] == sum(int(line[3]) for line in run.log if line[8] == "nni")
    assert s["ml_search_rounds"] == sum(1 for line in run.log if int(line[3]) > 0)


def test_the_scan_counts_the_listers_candidates(runs):
    """The first scan of a run sees the tree the plain run ends with: its candidates are the lister's on that tree."""
    for fam in ("spr8", "sim8"):
        names, parent, _ = R.from_newick(runs[fam, None].tree)
        for radius in (2, 4):
            first = [line for line in runs[fam, radius].log if line[8] == "spr"][0]
            assert int(first[1]) == len(S.candidates(len(names), parent, radius)), (fam, radius)


def test_simulated_family_needs_the_scan(runs):
    """One SPR of 4 edges from the generating tree: the interchanges alone end elsewhere, the search with --ml_spr 4 ends on the
    generating tree's bipartitions through an applied spr line whose single move has the gain a full evaluation confirms; radius 2
    does not reach that far."""
    plain, run = runs["spr8", None], runs["spr8", 4]
    assert N.bipartitions(plain.tree) != N.bipartitions(TRUE8)
    assert N.bipartitions(run.tree) == N.bipartitions(TRUE8) and N.bipartitions(runs["spr8", 2].tree) != N.bipartitions(TRUE8)
    applied = [line for line in run.log if line[8] == "spr" and int(line[3]) > 0]
    assert len(applied) == 1 and int(applied[0][3]) == 1 and run.stats["ml_lnl"] > plain.stats["ml_lnl"] + 10
    # exactly one scan applied exactly one move, so the tie of rho to a full evaluation (test_log_with_the_flag) is exercised: here too
    before, there, gain = float(applied[0][5]), float(applied[0][6]), float(applied[0][4])
    assert gain > 10 and abs((there - before) - gain) <= 1e-9 * abs(before)
    start = R.from_newick(SPR_START)
    back = [tuple(x) for x in S.candidates(8, start[1], 4).tolist()]
    lens = {len(p[0]) - 1 + len(p[1]) for p in (S.path_of(start[1], v, y) for v, y in back)}
    assert 4 in lens
    moved = [(v, y) for v, y in back if N.bipartitions(regrafted_newick(start, v, y)) == N.bipartitions(TRUE8)]
    assert moved and all(len(S.path_of(start[1], v, y)[0]) - 1 + len(S.path_of(start[1], v, y)[1]) >= 3 for v, y in moved)


def regrafted_newick(tree, v, y):
    names, parent, _ = tree
    parent2, _ = S.regrafted(len(names), parent, v, y)
    return N.newick_of(names, parent2, np.ones(len(parent2) - 1))


def test_beside_the_other_flags(exe, fams, tmp_path):
    """--ml_gamma 4, --ml_nni_opt 3 and --ml_support beside the flag: the runs end, their logs hang together, lnL is never below the
    run's without --ml_spr, and the other flags' own keys and files are there."""
    base = DNA(fams)
    for tag, extra in (("gamma", ["--ml_gamma", "4"]), ("opt", ["--ml_nni_opt", "3"])):
        plain = TS.run_s(exe, fams["spr8"], tmp_path, tag + "_plain", base + extra, search=20, start=fams["spr_start"])
        run = TS.run_s(exe, fams["spr8"], tmp_path, tag, base + extra + ["--ml_spr", "4"], search=20, start=fams["spr_start"])
        assert run.stats["ml_lnl"] >= plain.stats["ml_lnl"] and hangs_together(run.log) == run.stats["ml_lnl"], tag
        kinds = [line[8] for line in run.log]
        first = kinds.index("spr")
        assert [line[:8] for line in run.log[:first]] == plain.log[:first] and len(plain.log) == first, tag
        assert N.bipartitions(run.tree) == N.bipartitions(TRUE8), tag
        assert run.stats["ml_spr_calls"] >= 1 and run.stats["ml_spr_candidates"] > 0   # (the scan ran; under these flags the interchanges may get there alone)
        if tag == "opt":
            assert run.stats["ml_nni_opt_calls"] >= plain.stats["ml_nni_opt_calls"] > 0
    sup = TSUP.run_sup(exe, fams["spr8"], tmp_path, "sup", base + ["--ml_start", fams["spr_start"], "--ml_search", "20", "--ml_spr", "4"], reps=50)
    assert sup.stats["ml_spr_applied"] >= 1 and len(sup.nodes) in (4, 5)   # (the inner nodes below the children of the binary root, one of which may be a leaf)
    assert N.bipartitions(sup.tree) == N.bipartitions(TRUE8)
