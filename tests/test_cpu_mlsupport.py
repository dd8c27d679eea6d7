"""`--ml_support` and its companions through the CPU oracle driver (pgmsa_oracle: Backend::resampled_sums's default, the host loop), and
the pieces below it:
  - tests/resample_ref.py itself against brute force (every replicate's gathered alignment on the tree and on the exchanged tree,
    both evaluated by treelik_rates_ref);
  - resampled_sums_host, bootstrap_columns and ml_branch_support in a stand-alone program (tests/native/resample_test.cpp), its %a
    output equal to the statement bit for bit; built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, runs without the flags, the files' shapes, and what the values say on simulated families."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import resample_ref as RS
import test_cpu_bootstrap as TB
import test_cpu_mlancestral as TA
import test_cpu_mlsearch as TS
import test_cpu_mltree as TM
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 256.0 * math.log(2.0)


# ---- the statement against brute force ---------------------------------------------------------------------------------------------------
def full_lnl(dim, nleaves, parent, rows, pi, w, P):
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    return float(np.sum(np.log(out["site_l"]) - STEP * out["site_k"]))


def support_case(dim, tree, ncat, seed, nrep=4):
    """TS.generator_case with the candidates of the supported nodes alone, and nrep replicates of --bootstrap's columns."""
    case = dict(TS.generator_case(dim, tree, ncat, seed))
    nodes, cand = RS.supported(case["nleaves"], case["parent"])
    case.update(nodes=nodes, cand=cand, cols=RS.columns(nrep, case["rows"].shape[1], seed),
                want=N.evaluate(dim, case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], cand))
    return case


@pytest.mark.parametrize("dim,tree,ncat", [(dim, tree, ncat) for dim in (4, 20) for tree in ("balanced8", "inner3") for ncat in (1, 4)])
def test_resampled_gains_against_brute_force(dim, tree, ncat):
    """D[q][r] is the log-likelihood of the exchanged tree minus that of the tree, both on replicate r's alignment.  The bound is
    relative to |lnL| of the replicate, the measure DESIGN 3.20 takes for best_gain: the largest deviation measured over these 8
    cases is 3.14e-16, asserted: ten times that.  The identity columns give treelik_nni_gain bit for bit."""
    case = support_case(dim, tree, ncat, 500 + dim + ncat + sum(map(ord, tree)))
    nleaves, parent, rows, pi, w, P, cand, cols = (case[k] for k in ("nleaves", "parent", "rows", "pi", "w", "P", "cand", "cols"))
    kids = R.children_of(parent)
    root = len(parent) - 1
    assert case["nodes"] == [v for v in range(nleaves, root) if not (int(parent[v]) == root and len(kids[root]) == 2)]
    assert len(cand) == sum(len(kids[v]) * (len(kids[int(parent[v])]) - 1) for v in case["nodes"]) > 0
    rho = case["want"]["rho"]
    D = RS.sums(RS.log_rho(rho), cols)
    nedges = len(parent) - 1
    Pm = np.asarray(P).reshape(ncat, nedges, dim * dim)
    worst = 0.0
    for r in range(len(cols)):
        gathered = np.ascontiguousarray(rows[:, cols[r]])
        here = full_lnl(dim, nleaves, parent, gathered, pi, w, P)
        for q, (v, a, c) in enumerate(cand):
            parent2, old = N.exchanged(nleaves, parent, int(v), int(a), int(c))
            there = full_lnl(dim, nleaves, parent2, gathered, pi, w, np.ascontiguousarray(Pm[:, old[:nedges], :]).reshape(-1))
            worst = max(worst, abs(D[q, r] - (there - here)) / abs(here))
    print("largest deviation relative to |lnL|: %.3g" % worst)
    assert worst <= 3.14e-15
    identity = np.arange(rows.shape[1], dtype=np.uint32)[None, :]
    assert R.same_bits(RS.sums(RS.log_rho(rho), identity)[:, 0], N.gain(rho))


def test_statistics_on_hand_made_ratios():
    """Two nodes of two candidates each, three columns, replicates chosen by hand: a candidate of gain -infinity is dropped, a node
    left with none has alrt = +inf and full support, ties go to the tree, equal largest values give a gap of 0."""
    e = math.exp
    rho = np.array([[e(-1.0), e(-2.0), e(0.5)],     # node 8: gains -2.5 and -infinity
                    [1.0, 0.0, 1.0],
                    [0.0, 1.0, 1.0],                # node 9: both -infinity
                    [1.0, 1.0, 0.0]])
    cand = np.array([[8, 0, 2], [8, 1, 2], [9, 2, 0], [9, 3, 0]], np.uint32)
    cols = np.array([[0, 1, 2], [2, 2, 2], [0, 0, 0], [1, 1, 1]], np.uint32)
    (n8, k8, alrt8, sh8, rell8), (n9, k9, alrt9, sh9, rell9) = RS.statistics([8, 9], cand, rho, cols)
    assert (n8, k8, n9, k9) == (8, 2, 9, 2)
    assert alrt8 == 2 * -(math.log(e(-1.0)) + math.log(e(-2.0)) + math.log(e(0.5)))
    # D of the one candidate left: -2.5, 1.5, -3, -6; mean -2.5; e: 0, 4, -0.5, -3.5; gaps 0 (tie), 4, 0.5, 3.5 against d_obs 2.5
    assert sh8 == 2 and rell8 == 3
    assert (alrt9, sh9, rell9) == (math.inf, 4, 4)
    # d_obs <= 0: no SH hit whatever the gaps
    better = RS.statistics([8], cand[:1], np.array([[e(1.0), 1.0, 1.0]]), cols)
    assert better[0][2] == -2.0 and better[0][3] == 0 and better[0][4] == 2


# ---- the host code, stand-alone ----------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_mlsupport.py, which takes these lists from here: the host loop runs every one of them.
SUM_CASES = [s + ("random",) for s in RS.SHAPES] + [(65, 17, 5, kind) for kind in RS.KINDS[1:]] + [(4 * RS.T + 1, 257, 65, kind) for kind in ("minus infinity", "mixed magnitude")]
SUPPORT_CASES = [(dim, 33, "balanced8", ncat) for dim in (4, 20) for ncat in (1, 4)] + [(4, 17, "inner3", 2), (20, 17, "trifurcating", 2), (4, 15, "four", 2), (4, 15, "three", 2)]
SUPPORT_REPS = 25


def sum_bytes(nrow, ncols, nrep, x, cols, nulls=0):
    return b"".join([np.array([0, nrow, ncols, nrep, x.size, cols.size, nulls], np.int32).tobytes(), np.ascontiguousarray(x, np.float64).tobytes(),
                     np.ascontiguousarray(cols, np.uint32).tobytes()])


def bad_sum_blobs():
    x, cols, _ = RS.make_case(3, 5, 2)
    none = np.zeros(0)
    bad = [sum_bytes(3, 5, 2, x, cols, nulls) for nulls in (1, 2, 4)]
    bad += [sum_bytes(0, 5, 2, none, cols), sum_bytes(3, 0, 2, none, none), sum_bytes(3, 5, 0, x, none)]
    bad += [sum_bytes(65536, 1, 65536, none, none), sum_bytes(1, 65536, 65536, none, none)]   # nrow * nrep, nrep * ncols beyond 32 bits
    bad += [sum_bytes(3, 5, 2, xx, cc) for xx, cc in RS.bad_calls()]
    return bad


def support_inputs(key):
    c = N.make_case(*key)
    nodes, cand = RS.supported(c["nleaves"], c["parent"])
    cols = RS.columns(SUPPORT_REPS, c["rows"].shape[1], 11 + key[0])
    rho = N.evaluate(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"], cand)["rho"] if len(cand) else np.zeros((0, c["rows"].shape[1]))
    return c, nodes, cand, cols, rho


def dropped_case(both):
    """((0, 1)4, 2)5, 3)6 with matrices that hold zeros, so that a neighbour is impossible where the tree is not: leaf 2 keeps the
    state of node 5, node 4 has that state + 1, leaf 0 the state of node 4 or the next (`both`: exactly that of node 4), and row 0 =
    row 2 + 1 in every column.  Candidate (4, 0, 2) then has rho = 0 everywhere and is dropped; (4, 1, 2) is possible, unless `both`:
    then node 4 is left with no candidate."""
    base = N.make_case(4, 15, "four", 1)
    parent = np.array([4, 4, 5, 6, 5, 6, R.ROOT], np.uint32)
    rng = np.random.default_rng(77 + both)
    P0 = rng.uniform(0.01, 1.0, (6, 4, 4))
    P0 /= P0.sum(axis=2, keepdims=True)
    eye, shift = np.eye(4), np.roll(np.eye(4), 1, axis=1)
    assert shift[0, 1] == 1.0
    P0[0] = eye if both else 0.5 * (eye + shift)
    P0[2], P0[4] = eye, shift
    rows = rng.integers(0, 4, (4, 15)).astype(np.int8)
    rows[0] = (rows[2] + 1) % 4
    c = dict(dim=4, nleaves=4, parent=parent, rows=rows, pi=base["pi"], w=base["w"], P=R.pack(P0[:, None]), tree="dropped, both" if both else "dropped", ncat=1)
    nodes, cand = RS.supported(4, parent)
    assert nodes == [4] and cand.tolist() == [[4, 0, 2], [4, 1, 2]]
    cols = RS.columns(SUPPORT_REPS, 15, 5)
    rho = N.evaluate(4, 4, parent, rows, c["pi"], c["w"], c["P"], cand)["rho"]
    assert np.all(rho[0] == 0.0) and (np.all(rho[1] == 0.0) if both else np.all(rho[1] > 0.0))
    return c, nodes, cand, cols, rho


def support_bytes(c, cols, x_bytes):
    head = np.array([2, c["dim"], c["nleaves"], len(c["parent"]), c["rows"].shape[1], c["ncat"], len(cols), x_bytes], np.int32)
    parts = [head, np.asarray(c["parent"], np.uint32), np.asarray(c["rows"], np.int8), np.asarray(c["pi"], np.float64), np.asarray(c["w"], np.float64),
             np.asarray(c["P"], np.float64), np.asarray(cols, np.uint32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("resample_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "resample_test.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    blobs = []
    for nrow, ncols, nrep, kind in SUM_CASES:
        x, cols, _ = RS.make_case(nrow, ncols, nrep, kind)
        blobs.append(sum_bytes(nrow, ncols, nrep, x, cols))
    bad = bad_sum_blobs()
    blobs += bad
    blobs.append(np.array([1, 2, 41, 77], np.int32).tobytes())   # the columns of two replicates of 41 columns, seed 77
    support = [dropped_case(False), dropped_case(True)] + [support_inputs(key) for key in SUPPORT_CASES]
    for c, nodes, cand, cols, rho in support:
        blobs.append(support_bytes(c, cols, 1 << 30))
        blobs.append(support_bytes(c, cols, 1))   # (a row per resampled_sums call)
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(blobs)], np.int32).tobytes())
        for b in blobs:
            f.write(b)
    # (-fno-sanitize=vptr: as tests/test_cpu_mltree.py, the unit holds Backend's virtual defaults without the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("resample_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    for name in flags:
        r = subprocess.run([str(d / ("resample_test_" + name)), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % len(blobs)), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    return SimpleNamespace(bad=bad, support=support, lines=out)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_code_equals_the_statement(native, build):
    lines = native.lines[build]
    floats = lambda text: np.array([float.fromhex(v) for v in text.split()])
    for k, key in enumerate(SUM_CASES):
        want = RS.make_case(*key)[2]
        assert not np.any(np.isnan(want)), key
        assert R.same_bits(floats(lines[k]).reshape(want.shape), want), (build, key)
    at = len(SUM_CASES)
    rejected = lines[at:at + len(native.bad)]
    assert len(rejected) == len(native.bad) and all(line.startswith("rejected resampled sums: ") for line in rejected), rejected
    at += len(native.bad)
    # the shared generator: what tests/test_cpu_bootstrap.py's restatement of --bootstrap's stream draws
    assert [int(v) for v in lines[at].split()] == TB.resampled_columns(77, 2, 41).reshape(-1).tolist() == RS.columns(2, 41, 77).reshape(-1).tolist()
    at += 1
    some_sh = set()
    for c, nodes, cand, cols, rho in native.support:
        want = RS.statistics(nodes, cand, rho, cols)
        for _ in range(2):   # within the byte bound in one call, then a row a call
            got = lines[at:at + len(want) + 1]
            at += len(want) + 1
            assert got[-1] == "end %d" % len(want), (build, c["tree"], got)
            for line, (v, ncand, alrt, sh, rell) in zip(got, want):
                f = line.split()
                assert [int(f[0]), int(f[1]), int(f[3]), int(f[4])] == [v, ncand, sh, rell] and float.fromhex(f[2]) == alrt, (build, c["tree"], line, alrt)
                some_sh.add(sh); some_sh.add(rell)
    assert lines[at] == "ok %d cases" % (len(SUM_CASES) + len(native.bad) + 1 + 2 * len(native.support)) and len(lines) == at + 1
    first, second = (RS.statistics(nodes, cand, rho, cols) for c, nodes, cand, cols, rho in native.support[:2])
    assert first[0][1] == 2 and math.isfinite(first[0][2]) and second[0][1:] == (2, math.inf, SUPPORT_REPS, SUPPORT_REPS)   # (one candidate dropped; both)
    assert len(some_sh - {0, SUPPORT_REPS}) >= 3   # (the cases reach counts between none and all)
    # the trees of 3 and of 4 leaves have a binary root alone above their inner nodes: no supported node
    assert [len(nodes) for c, nodes, _, _, _ in native.support[-2:]] == [0, 0]


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


ZERO8 = TS.TRUE8.replace("(t1:0.1,t2:0.15):0.12", "(t1:0.1,t2:0.15):0.0")   # the branch above (t1, t2) has length 0: its resolution is arbitrary
TRI8 = "((t1:0.1,t2:0.15):0.12,(t3:0.2,t4:0.1):0.2,((t5:0.12,t6:0.18):0.25,(t7:0.1,t8:0.2):0.3):0.25);"   # TRUE8 with a trifurcating root
CUT = 0.75   # between the two groups measured at N = 1000: every true branch 1.0 and 1.0, the arbitrary one 0.0 and at most 0.46


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlsup_fams")
    aa = bu.aa_families(d)
    out = dict(aa5=[f for f in aa if f.endswith("_n5.fa")][0], aa8=[f for f in aa if f.endswith("_n8.fa")][0], hky=bu.hky_model(d), dir=d)
    hky = R.custom(out["hky"], 4)
    for seed in (1, 2, 3):
        out["sim8_%d" % seed] = os.path.join(str(d), "sim8_%d.fa" % seed)
        TS.simulate_dna(out["sim8_%d" % seed], hky, TS.TRUE8, seed, 2000)
    out["sim8"] = out["sim8_1"]
    out["zero8"] = os.path.join(str(d), "zero8.fa")
    TS.simulate_dna(out["zero8"], hky, ZERO8, 1, 2000)
    for name, text in (("true", TS.TRUE8), ("one", TS.ONE_AWAY), ("zero", ZERO8), ("tri", TRI8)):
        out[name] = TS.write(os.path.join(str(d), name + ".nwk"), text)
    three = TM.parse_fasta(open(out["aa5"]).read())
    out["aa3"] = os.path.join(str(d), "aa3.fa")
    with open(out["aa3"], "w") as f:
        for n in sorted(three)[:3]:
            f.write(">%s\n%s\n" % (n, three[n]))
    return out


def run_sup(exe, fa, d, tag, opts=(), reps=None, seed=None, table=True, env=None):
    """A run with --ml_support (and --ml_ancestral_tree, whose names the table takes); r.nodes: the table's lines as (name, candidates,
    alrt, sh_hits, rell_hits)."""
    p = {k: os.path.join(str(d), "%s.%s" % (tag, k)) for k in ("support", "table")}
    extra = ["--ml_support", p["support"]] + (["--ml_support_table", p["table"]] if table else [])
    extra += (["--ml_support_reps", str(reps)] if reps is not None else []) + (["--ml_support_seed", str(seed)] if seed is not None else [])
    r = TA.run_a(exe, fa, d, tag, ["-i", "0"] + list(opts) + extra, probs=False, env=env)
    for k in p:
        setattr(r, k, open(p[k]).read() if os.path.exists(p[k]) else None)
    r.nodes = None
    if r.table is not None:
        lines = r.table.splitlines()
        r.head = lines[:2]
        r.nodes = [(f[0], int(f[1]), float(f[2]), int(f[3]), int(f[4])) for f in (line.split("\t") for line in lines[2:])]
        assert all(len(line.split("\t")) == 5 for line in lines[2:])
    return r


DNA = TS.DNA


def test_refusals(exe, fams, tmp_path):
    fa = fams["aa5"]
    tree, sup, tab = str(tmp_path / "never.tree"), str(tmp_path / "never.sup"), str(tmp_path / "never.tab")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    ml, s = ["--ml_tree", tree], ["--ml_support", sup]
    cases = [
        (s + [fa], "need --ml_tree"),
        (["--ml_support_table", tab, fa], "need --ml_tree"),
        (["--ml_support_reps", "10", fa], "need --ml_tree"),
        (["--ml_support_seed", "3", fa], "need --ml_tree"),
        (ml + ["--ml_support_table", tab, fa], "need --ml_support"),
        (ml + ["--ml_support_reps", "10", fa], "need --ml_support"),
        (ml + ["--ml_support_seed", "3", fa], "need --ml_support"),
        (ml + s + [fams["aa3"]], "--ml_support needs at least 4 sequences"),
        (ml + s + ["-W", fa], "cannot be combined with -W"),
        (ml + s + ["-r", fa], "cannot be combined with -r"),
        (ml + s + ["--topology", fams["true"], fa], "cannot be combined with --topology"),
        (ml + s + ["--batch", lst], "--batch cannot be combined"),
        (ml + s + ["--ml_gamma", "1", fa], "--ml_gamma takes"),
        (ml + s + ["--ml_rounds", "0", fa], "--ml_rounds takes"),
        (ml + s + ["--ml_start", str(tmp_path / "absent.nwk"), fa], "cannot open"),
    ]
    for text in ("0", "10001", "-1", "abc", "1.5", "", "3x"):
        cases.append((ml + s + ["--ml_support_reps", text, fa], "--ml_support_reps takes a number of replicates from 1 to 10000"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta", "-i", "0"] + args, code=2)
        assert "ERROR:" in r.stderr and message in r.stderr, (args, r.stderr)
        assert r.stdout == "" and not any(os.path.exists(p) for p in (tree, sup, tab)), args


def test_runs_without_the_flags_are_unchanged(exe, fams, tmp_path):
    """No key of the support among the stats without the flag, and the other files are the same with and without it."""
    plain = TA.run_a(exe, fams["aa8"], tmp_path, "plain", ["-i", "0"], probs=False)
    assert not any(k.startswith("ml_support") for k in plain.stats)
    with_it = run_sup(exe, fams["aa8"], tmp_path, "with", reps=10)
    assert (with_it.stdout, with_it.tree, with_it.sites, with_it.anc, with_it.anctree) == (plain.stdout, plain.tree, plain.sites, plain.anc, plain.anctree)
    same = lambda a, b: {k: v for k, v in a.items() if not k.endswith("_s") and not k.startswith("ml_support")} == {k: v for k, v in b.items() if not k.endswith("_s")}
    assert same(with_it.stats, plain.stats)
    assert with_it.stats["ml_support_nodes"] == len(with_it.nodes) and with_it.stats["ml_support_calls"] == 1 and with_it.stats["ml_support_s"] > 0
    assert with_it.stats["ml_support_kernel_ms"] == 0


def check_shapes(r, reps, seed):
    """The table against the labelled trees: the names are --ml_ancestral_tree's, the nodes at a binary root are absent, every other
    inner node below the root is there in node order, the support tree labels exactly those nodes with %.6f of sh_hits / N."""
    assert r.head == ["replicates\t%d" % reps, "seed\t%d" % seed]
    names, parent, lengths, labels = TA.labelled_newick(r.anctree)
    nleaves, root = len(names), len(parent) - 1
    nodes, cand = RS.supported(nleaves, parent)
    assert [n[0] for n in r.nodes] == [labels[v - nleaves] for v in nodes] == ["N%d" % (v - nleaves + 1) for v in nodes]
    assert [n[1] for n in r.nodes] == [int(np.sum(cand[:, 0] == v)) for v in nodes]
    assert all(0 <= n[3] <= reps and 0 <= n[4] <= reps for n in r.nodes)
    snames, sparent, slengths, slabels = TA.labelled_newick(r.support)
    assert (snames, sparent.tolist(), slengths.tolist()) == (names, parent.tolist(), lengths.tolist())
    want = {v: "%.6f" % (n[3] / reps) for v, n in zip(nodes, r.nodes)}
    assert slabels == [want.get(v, "") for v in range(nleaves, root + 1)]
    assert TS.T_strip(r.support) == r.tree.strip()
    return nodes, parent


def test_file_shapes_seeds_and_one_replicate(exe, fams, tmp_path):
    r = run_sup(exe, fams["aa8"], tmp_path, "a", reps=50, seed=5)
    nodes, parent = check_shapes(r, 50, 5)
    kids = R.children_of(parent)
    root = len(parent) - 1
    assert len(kids[root]) == 2 and not set(nodes) & set(kids[root]) and len(nodes) == len(parent) - 8 - 1 - sum(1 for c in kids[root] if c >= 8)
    again = run_sup(exe, fams["aa8"], tmp_path, "b", reps=50, seed=5)
    assert (again.support, again.table) == (r.support, r.table)
    other = run_sup(exe, fams["aa8"], tmp_path, "c", reps=50, seed=6)
    assert [n[2] for n in other.nodes] == [n[2] for n in r.nodes]   # (the aLRT does not depend on the replicates)
    assert [n[3:] for n in other.nodes] != [n[3:] for n in r.nodes]
    default = run_sup(exe, fams["aa8"], tmp_path, "d")
    check_shapes(default, 1000, 1)
    one = run_sup(exe, fams["aa8"], tmp_path, "e", reps=1)
    check_shapes(one, 1, 1)
    assert all(n[3] in (0, 1) and n[4] in (0, 1) for n in one.nodes)
    no_table = run_sup(exe, fams["aa8"], tmp_path, "f", reps=50, seed=5, table=False)
    assert no_table.support == r.support and no_table.table is None


def test_trifurcating_root_and_a_tree_without_supported_nodes(exe, fams, tmp_path):
    """Under a trifurcating --ml_start root the root's inner children are supported, with 4 candidates each; 4 taxa under a binary root
    have no supported node: the tree unlabelled and a table of the two header lines."""
    r = run_sup(exe, fams["sim8"], tmp_path, "tri", DNA(fams) + ["--ml_start", fams["tri"]], reps=20)
    nodes, parent = check_shapes(r, 20, 1)
    kids = R.children_of(parent)
    root = len(parent) - 1
    assert len(kids[root]) == 3 and set(kids[root]) <= set(nodes) and len(nodes) == 5
    assert [n[1] for v, n in zip(nodes, r.nodes) if int(parent[v]) == root] == [4, 4, 4]
    names = sorted(TM.parse_fasta(open(fams["aa5"]).read()))[:4]
    four = os.path.join(str(tmp_path), "four.fa")
    seqs = TM.parse_fasta(open(fams["aa5"]).read())
    with open(four, "w") as f:
        for n in names:
            f.write(">%s\n%s\n" % (n, seqs[n]))
    start = TS.write(tmp_path / "four.nwk", "((%s:0.1,%s:0.1):0.1,(%s:0.1,%s:0.1):0.1);" % tuple(names))
    r = run_sup(exe, four, tmp_path, "four", ["--ml_start", start], reps=20)
    assert r.table == "replicates\t20\nseed\t1\n" and r.support == r.tree and r.stats["ml_support_nodes"] == 0 and r.stats["ml_support_calls"] == 0


@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"], ["--ml_search", "5"]])
def test_with_gamma_and_with_the_search(exe, fams, tmp_path, opts):
    """The flags describe whatever tree the run ends with: plain, under --ml_gamma 4 (rho is the mixture's), and behind --ml_search."""
    r = run_sup(exe, fams["sim8"], tmp_path, "s", DNA(fams) + ["--ml_start", fams["one"]] + opts, reps=50)
    check_shapes(r, 50, 1)
    assert ("ml_search_s" in r.stats) == ("--ml_search" in opts)
    if "--ml_gamma" in opts:
        assert r.stats["ml_categories"] == 4
    assert all(math.isfinite(n[2]) for n in r.nodes)
    if "--ml_search" in opts:
        assert N.bipartitions(r.tree) == N.bipartitions(TS.TRUE8) and all(n[2] > 0 for n in r.nodes)


def test_true_branches_are_high_and_an_arbitrary_one_is_low(exe, fams, tmp_path):
    """8 taxa x 2000 simulated nucleotide columns.  On the generating topology (seeds 1 .. 3) every supported node has sh and rell 1.0
    at N = 1000 (measured on this driver: 1000 of 1000 hits at all 12 nodes, aLRT 235 .. 1068).  With the branch above (t1, t2) of
    length 0 in the simulation that node has sh 0.0 and rell 0.131 (seeds 1 .. 5: sh 0.0, rell 0.069 .. 0.460; aLRT -0.18 .. -2e-4) and
    the other three stay at 1.0.  One cut, 0.75, lies between the groups."""
    for seed in (1, 2, 3):
        r = run_sup(exe, fams["sim8_%d" % seed], tmp_path, "true%d" % seed, DNA(fams) + ["--ml_start", fams["true"]])
        check_shapes(r, 1000, 1)
        print(seed, r.nodes)
        assert len(r.nodes) == 4 and all(n[3] > CUT * 1000 and n[4] > CUT * 1000 and n[2] > 0 for n in r.nodes)
    z = run_sup(exe, fams["zero8"], tmp_path, "zero", DNA(fams) + ["--ml_start", fams["zero"]])
    print(z.nodes)
    assert N.bipartitions(z.tree) == N.bipartitions(ZERO8) and [n[0] for n in z.nodes] == ["N1", "N2", "N4", "N5"]
    assert z.nodes[0][3] < CUT * 1000 and z.nodes[0][4] < CUT * 1000
    assert all(n[3] > CUT * 1000 and n[4] > CUT * 1000 for n in z.nodes[1:])


def test_a_wrong_branch_has_a_negative_statistic(exe, fams, tmp_path):
    """From one interchange away without the search, the node whose edge is wrong has a better neighbour: d_obs < 0, so alrt < 0 and
    sh_hits = 0 there; with the search the same start ends on the generating topology and every node is high."""
    r = run_sup(exe, fams["sim8"], tmp_path, "wrong", DNA(fams) + ["--ml_start", fams["one"]], reps=200)
    assert N.bipartitions(r.tree) == N.bipartitions(TS.ONE_AWAY)
    wrong = [n for n in r.nodes if n[2] < 0]
    assert len(wrong) == 1 and wrong[0][3] == 0 and wrong[0][4] == 0
    found = run_sup(exe, fams["sim8"], tmp_path, "found", DNA(fams) + ["--ml_start", fams["one"], "--ml_search", "10"], reps=200)
    assert N.bipartitions(found.tree) == N.bipartitions(TS.TRUE8)
    assert all(n[2] > 0 and n[3] > CUT * 200 and n[4] > CUT * 200 for n in found.nodes)


def test_host_switches_do_not_change_the_oracle_driver(exe, fams, tmp_path):
    base = run_sup(exe, fams["sim8"], tmp_path, "base", DNA(fams), reps=50)
    for switch in ("PGM_HOST_TREELIK", "PGM_DEVICE_TREELIK"):   # (this driver's backend has the default body: the host loop either way)
        r = run_sup(exe, fams["sim8"], tmp_path, switch, DNA(fams), reps=50, env=dict(os.environ, **{switch: "1"}))
        assert (r.tree, r.support, r.table) == (base.tree, base.support, base.table) and r.stats["ml_support_kernel_ms"] == 0
