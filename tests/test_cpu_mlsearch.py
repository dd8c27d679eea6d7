"""`--ml_search`, `--ml_start` and `--ml_search_log` through the CPU oracle driver (pgmsa_oracle: Backend::tree_nni's default, the host
loop), and the pieces below it:
  - tests/treelik_nni_ref.py itself against brute force (every candidate's exchanged tree evaluated by treelik_rates_ref);
  - tree_nni_host and treelik_nni_gain in a stand-alone program (tests/native/treelik_nni_test.cpp), its %a output equal to the
    statement bit for bit; built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, runs without the flags, --ml_start, the search on simulated families, its log, the local optimum."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import mldist_general_ref as M
import test_cpu_mlancestral as TA
import test_cpu_mlgamma as TG
import test_cpu_mltree as TM
import test_cpu_treelik_shapes as SH
import transfer_ref as T
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 256.0 * math.log(2.0)
EPSILON = 1e-4   # the default of --ml_epsilon


# ---- the statement against brute force ---------------------------------------------------------------------------------------------------
def brute_log_ratio(case, q):
    """log of L'_s 2^(-256 k'_s) / (L_s 2^(-256 k_s)) for candidate q: the exchanged tree, renumbered children before parents, every
    edge with the matrices of the node it hangs below, evaluated by treelik_rates_ref."""
    dim, nleaves, parent, ncat = case["dim"], case["nleaves"], case["parent"], case["ncat"]
    nedges = len(parent) - 1
    v, a, c = (int(x) for x in case["cand"][q])
    parent2, old = N.exchanged(nleaves, parent, v, a, c)
    P = np.asarray(case["P"]).reshape(ncat, nedges, dim * dim)
    P2 = np.ascontiguousarray(P[:, old[:nedges], :]).reshape(-1)
    there = G.evaluate(dim, nleaves, parent2, case["rows"], case["pi"], case["w"], P2, derivs=False)
    here = case["want"]
    with np.errstate(divide="ignore"):
        return (np.log(there["site_l"]) - STEP * there["site_k"]) - (np.log(here["site_l"]) - STEP * here["site_k"]), there, here


def generator_case(dim, tree, ncat, seed):
    """A case whose matrices are exp(Q r t) of a seeded generator that is not reversible; columns with gaps and -2."""
    nleaves, parent = N.TREES[tree]()
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
    cand = N.candidates(nleaves, parent)
    return dict(dim=dim, nleaves=nleaves, parent=parent, rows=rows, pi=pi, w=w, P=P, tree=tree, ncat=ncat, cand=cand,
                want=N.evaluate(dim, nleaves, parent, rows, pi, w, P, cand))


BRUTE = [(dim, tree, ncat) for dim in (4, 20) for tree in ("balanced8", "trifurcating", "inner3") for ncat in (1, 4)]


@pytest.mark.parametrize("dim,tree,ncat", BRUTE)
def test_reference_against_brute_force(dim, tree, ncat):
    """Every candidate of the balanced tree of 8, of the trifurcating root and of the tree with an inner trifurcation, under a
    generator that is not reversible: rho within 1e-10 relative of the ratio of the two trees' site likelihoods (the bound
    tests/test_cpu_mltree.py takes for its own brute-force check; measured here: below 4e-15)."""
    case = generator_case(dim, tree, ncat, 300 + dim + ncat + sum(map(ord, tree)))
    want = case["want"]
    kids = R.children_of(case["parent"])
    if tree == "trifurcating":
        assert len(kids[len(case["parent"]) - 1]) == 3
    if tree == "inner3":
        assert len(kids[6]) == 3 and int(case["parent"][6]) != R.ROOT
    assert len(case["cand"]) == sum(len(kids[v]) * (len(kids[int(case["parent"][v])]) - 1) for v in range(case["nleaves"], len(kids) - 1))
    worst = 0.0
    for q in range(len(case["cand"])):
        log_ratio, there, here = brute_log_ratio(case, q)
        assert np.all(there["site_k"] == 0) and np.all(here["site_k"] == 0)
        ratio = there["site_l"] / here["site_l"]
        worst = max(worst, float(np.max(np.abs(want["rho"][q] - ratio) / ratio)))
    print("largest relative difference: %.3g" % worst)
    assert worst < 1e-10
    assert np.all(want["rho"][:, 2] > 0)   # (a column of gaps: every tree has likelihood 1 up to rounding)
    assert np.max(np.abs(want["rho"][:, 2] - 1)) < 1e-12


def test_caterpillar_scaling_in_log_space():
    """The caterpillar of 96 leaves, every matrix entry in [0.03, 0.07]: every rho is finite and above 0, some candidate has
    k_N != k_D on some column, and there log rho is within 1e-10 of the brute-force log ratio (the same bound, in log space)."""
    case = N.make_case(4, 17, "caterpillar96", 1)
    want = case["want"]
    assert np.all(np.isfinite(want["rho"])) and np.all(want["rho"] > 0)
    differs = np.argwhere((want["cat_kd"][0] != want["cat_kn"][0]).any(axis=1))[:, 0]
    assert len(differs) > 0
    worst = 0.0
    for q in list(differs[:6]) + list(differs[-6:]):
        log_ratio, there, here = brute_log_ratio(case, int(q))
        worst = max(worst, float(np.max(np.abs(np.log(want["rho"][q]) - log_ratio))))
    print("largest difference of log rho: %.3g" % worst)
    assert worst < 1e-10


def test_gain_is_the_sum_of_the_logs():
    rho = np.array([[1.0, 2.0, 0.5], [1.0, 0.0, 3.0], [4.0, 4.0, 4.0]])
    assert N.gain(rho).tolist() == [math.log(1.0) + math.log(2.0) + math.log(0.5), -math.inf, math.log(4.0) + math.log(4.0) + math.log(4.0)]


# ---- the host loop, stand-alone ----------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_mlsearch.py, which takes these lists from here: the host loop runs every one of them.
DIMS = (4, 20, 61, 64)
GRID = [(dim, ncols, "balanced8", ncat) for dim in DIMS for ncols in (1, 15, 16, 17, 33) for ncat in (1, 2, 4)]
SMALL_TREES = [(dim, 17, "three", 2) for dim in DIMS] + [(dim, 17, "four", 2, "root") for dim in DIMS]
ARITY = [(dim, 17, tree, 2) for dim in DIMS for tree in ("trifurcating", "inner3")]
LARGER = [(20, 33, "balanced24", 4), (4, 17, "caterpillar96", 1), (20, 17, "caterpillar96", 2)]
ORDER = [(4, 33, "balanced8", 4, "one"), (20, 17, "balanced8", 2, "shuffled"), (4, 33, "inner3", 4, "shuffled")]
SMALL_VALID = (4, 15, "balanced8", 2)   # what the rejections change
NATIVE_CASES = list(dict.fromkeys(GRID + SMALL_TREES + ARITY + LARGER + ORDER + [SMALL_VALID] + SH.NATIVE_NNI))   # (SH: the other dims, polytomies)


def leaf_case():
    """Candidates whose a or c is a leaf with a state, a gap or -2, and columns of gaps alone: ((0,1)4,2)5,3)6 with hand-made rows."""
    base = N.make_case(4, 15, "four", 2)
    parent = np.array([4, 4, 5, 6, 5, 6, R.ROOT], np.uint32)
    rows = np.array([[0, -1, -2, 1, -1, 2, 3, -1],
                     [1, 2, 3, -1, -1, -2, 0, -1],
                     [2, 2, -1, -2, -1, 0, 1, -1],
                     [3, -2, 0, 2, -1, -1, -2, -1]], np.int8)
    cand = N.candidates(4, parent)
    assert cand.tolist() == [[4, 0, 2], [4, 1, 2], [5, 2, 3], [5, 4, 3]]
    return dict(dim=4, nleaves=4, parent=parent, rows=rows, pi=base["pi"], w=base["w"], P=base["P"], tree="leaves", ncat=2, cand=cand,
                want=N.evaluate(4, 4, parent, rows, base["pi"], base["w"], base["P"], cand))


def many_candidates_case():
    """More candidates than a grid's second dimension holds (65535): the two candidates of the tree of 3 leaves, 70001 in turn, one
    column.  The expectation is that of the two, repeated."""
    base = N.make_case(20, 1, "three", 2)
    pick = np.arange(70001) % 2
    want = dict(base["want"])
    want["rho"] = np.ascontiguousarray(base["want"]["rho"][pick])
    return dict(base, cand=np.ascontiguousarray(base["cand"][pick]), want=want, tree="three, 70001 candidates")


def _case_bytes(c, **kw):
    d = dict(c); d.update(kw)
    nnodes = d.get("nnodes", len(d["parent"]))
    cand = np.asarray(d["cand"], np.uint32).reshape(-1, 3)
    head = np.array([d["dim"], d["nleaves"], nnodes, d["rows"].shape[1], d["ncat"], d.get("ncand", len(cand))], np.int32)
    parts = [head, np.asarray(d["parent"], np.uint32), np.asarray(d["rows"], np.int8), np.asarray(d["pi"], np.float64), np.asarray(d["w"], np.float64), np.asarray(d["P"], np.float64), cand]
    return b"".join(np.ascontiguousarray(x).tobytes() for x in parts)


def bad_candidates():
    """What the entry refuses among the candidates of the balanced tree of 8 (nodes 8 .. 13 inner below the root 14; 8 = (0, 1),
    9 = (2, 3), 10 = (8, 9)): v a leaf, the root, beyond the nodes; a not a child of v; c not a child of u; c == v; out of range."""
    return [[[3, 0, 1]], [[14, 10, 13]], [[15, 0, 1]], [[0xFFFFFFFF, 0, 1]], [[8, 2, 9]], [[8, 15, 9]], [[8, 0, 8]], [[8, 0, 2]], [[8, 0, 15]], [[8, 0, 13]],
            [[8, 0, 9], [8, 0, 8]]]


def _bad_cases():
    c = N.make_case(*SMALL_VALID)
    bad = [_case_bytes(c, cand=np.zeros((0, 3), np.uint32))]   # no candidate
    for cand in bad_candidates():
        bad.append(_case_bytes(c, cand=np.array(cand, np.uint32)))
    for ncat in (0, 17):
        bad.append(_case_bytes(c, ncat=ncat, w=np.full(ncat, 0.5), P=np.tile(c["P"][:len(c["P"]) // 2], ncat)))
    for v in (0.0, float("nan")):
        bad.append(_case_bytes(c, w=np.array([0.5, v])))
    for b in TM._bad_cases():
        bad.append(_case_bytes(c, parent=b["parent"], rows=b["rows"], cand=c["cand"][:1]))
    return bad


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("nni_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_nni_test.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    cases = [N.make_case(*k) for k in NATIVE_CASES] + [leaf_case(), many_candidates_case()]
    bad = _bad_cases()
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases) + len(bad)], np.int32).tobytes())
        for c in cases:
            f.write(_case_bytes(c))
        for blob in bad:
            f.write(blob)
    # (-fno-sanitize=vptr: as tests/test_cpu_mltree.py, the unit holds Backend's virtual defaults without the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("nni_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    for name in flags:
        r = subprocess.run([str(d / ("nni_test_" + name)), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % (len(cases) + len(bad))), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    # the plain build again, holding the pieces of one column chunk at a time: every case of 17 and of 33 columns takes 2 and 3 blocks
    r = subprocess.run([str(d / "nni_test_plain"), path, "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0
    out["plain, a block per chunk"] = r.stdout.splitlines()
    return SimpleNamespace(cases=cases, bad=bad, lines=out)


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
        assert R.same_bits(floats(gain), N.gain(want["rho"])), what
    first = 5 * len(cases)
    rejected = lines[first:first + len(native.bad)]
    assert len(rejected) == len(native.bad) and all(line.startswith("rejected tree ") for line in rejected), rejected
    assert sum(line.startswith("rejected tree nni:") for line in rejected) == 1 + len(bad_candidates())
    assert len(lines) == first + len(native.bad) + 1


def test_statement_properties():
    """site_l, site_k and post are the rates entry's; a column of gaps gives 1 within rounding; repeated candidates repeat their rows."""
    for key in [(4, 33, "balanced8", 4), (20, 17, "balanced8", 2, "shuffled"), (61, 17, "trifurcating", 2)]:
        c = N.make_case(*key)
        old = G.evaluate(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"], derivs=False)
        for k in ("site_l", "site_k", "post"):
            assert R.same_bits(c["want"][k], old[k]), (key, k)
        assert np.max(np.abs(c["want"]["rho"][:, 3] - 1)) < 1e-12   # (site 3 is all gaps; the matrices are row-stochastic)
    c = N.make_case(20, 17, "balanced8", 2, "shuffled")
    full = N.make_case(20, 17, "balanced8", 2)
    for q, cand in enumerate(c["cand"]):
        at = [tuple(x) for x in full["cand"].tolist()].index(tuple(cand.tolist()))
        assert R.same_bits(c["want"]["rho"][q], full["want"]["rho"][at])
    w = leaf_case()["want"]
    assert np.all(w["rho"][:, 4] == 1.0) or np.max(np.abs(w["rho"][:, 4] - 1)) < 1e-12
    assert np.all(np.isfinite(w["rho"])) and np.all(w["rho"] > 0)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


TRUE8 = "(((t1:0.1,t2:0.15):0.12,(t3:0.2,t4:0.1):0.2):0.15,((t5:0.12,t6:0.18):0.25,(t7:0.1,t8:0.2):0.3):0.1);"
# one interchange away: candidate (v = (t1, t2), a = t2, c = (t3, t4)) applied; two: the same and its like in the clade of t5 .. t8,
# whose edges share no node with the first's.  The two harder starts exchange t2 with t3 (and t6 with t7): two interchanges around
# adjacent edges each, both splits of a clade of four replaced.
ONE_AWAY = "(((t1:0.1,(t3:0.2,t4:0.1):0.2):0.12,t2:0.15):0.15,((t5:0.12,t6:0.18):0.25,(t7:0.1,t8:0.2):0.3):0.1);"
TWO_AWAY = "(((t1:0.1,(t3:0.2,t4:0.1):0.2):0.12,t2:0.15):0.15,((t5:0.12,(t7:0.1,t8:0.2):0.3):0.25,t6:0.18):0.1);"
SWAPPED_PAIR = "(((t1:0.1,t3:0.15):0.12,(t2:0.2,t4:0.1):0.2):0.15,((t5:0.12,t6:0.18):0.25,(t7:0.1,t8:0.2):0.3):0.1);"
SWAPPED_PAIRS = "(((t1:0.1,t3:0.15):0.12,(t2:0.2,t4:0.1):0.2):0.15,((t5:0.12,t7:0.18):0.25,(t6:0.1,t8:0.2):0.3):0.1);"
STARTS = {"one": (ONE_AWAY, 1), "two": (TWO_AWAY, 2), "swapped_pair": (SWAPPED_PAIR, 2), "swapped_pairs": (SWAPPED_PAIRS, 4)}   # (text, splits that differ)
TRUE6 = "(((t1:0.1,t2:0.15):0.12,t3:0.2):0.15,((t4:0.12,t5:0.18):0.2,t6:0.3):0.1);"
SEED8, SEED6, SEED5 = 1, 1, 6   # (chosen so that the checks below hold, verified on the CPU: see their docstrings)


def simulate_dna(path, model, tree, seed, ncols):
    """Nucleotide sequences evolved down `tree` (a newick line with lengths) under (Q, pi) without indels, seeded numpy."""
    from scipy.linalg import expm
    Q, pi = model
    rng = np.random.default_rng(seed)
    seqs = {}

    def down(node, states):
        if isinstance(node, str):
            seqs[node] = states
            return
        for kid, ln, _ in node:
            P = np.clip(expm(Q * float(ln[1:])), 0, None)
            P /= P.sum(axis=1, keepdims=True)
            u = rng.random(ncols)
            down(kid, (u[:, None] > np.cumsum(P[states], axis=1)).sum(axis=1).clip(0, 3))

    down(T.parse(tree), rng.choice(4, size=ncols, p=pi / pi.sum()))
    with open(path, "w") as f:
        for n in sorted(seqs):
            f.write(">%s\n%s\n" % (n, "".join("TCAG"[x] for x in seqs[n])))


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mls_fams")
    aa = bu.aa_families(d)
    out = dict(aa5=[f for f in aa if f.endswith("_n5.fa")][0], aa8=[f for f in aa if f.endswith("_n8.fa")][0], hky=bu.hky_model(d), dir=d)
    hky = R.custom(out["hky"], 4)
    out["sim8"] = os.path.join(str(d), "sim8.fa")
    simulate_dna(out["sim8"], hky, TRUE8, SEED8, 2000)
    out["sim6"] = os.path.join(str(d), "sim6.fa")
    simulate_dna(out["sim6"], hky, TRUE6, SEED6, 1000)
    out["sim5"] = os.path.join(str(d), "sim5.fa")
    TG.simulated_family(out["sim5"], R.shipped("wag.qmat"), seed=SEED5, ntaxa=5, ncols=300, shape=50.0)
    for name, text in [(k, v[0]) for k, v in STARTS.items()] + [("true", TRUE8)]:
        out[name] = os.path.join(str(d), name + ".nwk")
        with open(out[name], "w") as f:
            f.write(text + "\n")
    return out


def write(path, text):
    with open(str(path), "w") as f:
        f.write(text + "\n")
    return str(path)


def run_s(exe, fa, d, tag, opts=(), search=None, start=None, log=True, env=None, code=0):
    p = os.path.join(str(d), tag + ".log")
    extra = (["--ml_search", str(search)] if search is not None else []) + (["--ml_start", start] if start else []) + (["--ml_search_log", p] if log and search is not None else [])
    r = TM.run_ml(exe, fa, d, tag, ["-i", "0"] + list(opts) + extra, env=env)
    r.log = [line.split("\t") for line in open(p).read().splitlines()] if os.path.exists(p) else None
    r.log_text = open(p).read() if os.path.exists(p) else None
    return r


DNA = lambda fams: ["--dna", "--custom_model", fams["hky"]]


def test_refusals(exe, fams, tmp_path):
    fa = fams["aa5"]
    names = sorted(R.read_fasta(fa))
    tree, log = str(tmp_path / "never.tree"), str(tmp_path / "never.log")
    cat = lambda ns: ("(" * (len(ns) - 1) + ns[0] + "".join(":0.1,%s:0.1)" % n for n in ns[1:]) + ";")   # (a caterpillar; the parser wants lengths)
    good = write(tmp_path / "good.nwk", cat(names))
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    ml = ["--ml_tree", tree]
    cases = [
        (["--ml_search", "3", fa], "need --ml_tree"),
        (["--ml_start", good, fa], "need --ml_tree"),
        (["--ml_search_log", log, fa], "need --ml_tree"),
        (ml + ["--ml_search_log", log, fa], "--ml_search_log needs --ml_search"),
        (ml + ["--ml_start", str(tmp_path / "absent.nwk"), fa], "cannot open"),
        (ml + ["--ml_start", write(tmp_path / "fewer.nwk", cat(names[:-1])), fa], "are not the sequences"),
        (ml + ["--ml_start", write(tmp_path / "more.nwk", cat(names + ["extra"])), fa], "are not the sequences"),
        (ml + ["--ml_start", write(tmp_path / "other.nwk", cat(names[:-1] + ["other"])), fa], "are not the sequences"),
        (ml + ["--ml_start", write(tmp_path / "twice.nwk", cat(names[:-1] + [names[0]])), fa], "are not the sequences"),
        (ml + ["--ml_start", write(tmp_path / "single.nwk", "(((%s:0.1,%s:0.1):0.1,%s:0.1):0.1,((%s:0.1):0.1,%s:0.1):0.1);" % tuple(names)), fa], "one child"),
        (ml + ["--ml_search", "3", "-W", fa], "cannot be combined with -W"),
        (ml + ["--ml_search", "3", "-r", fa], "cannot be combined with -r"),
        (ml + ["--ml_search", "3", "--topology", good, fa], "cannot be combined with --topology"),
        (ml + ["--ml_search", "3", "--batch", lst], "--batch cannot be combined"),
        (ml + ["--ml_search", "3", "--ml_gamma", "1", fa], "--ml_gamma takes"),
    ]
    for text in ("0", "1001", "-1", "abc", "1.5", "", "3x"):
        cases.append((ml + ["--ml_search", text, fa], "--ml_search takes a number of rounds from 1 to 1000"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta", "-i", "0"] + args, code=2)
        assert "ERROR:" in r.stderr and message in r.stderr, (args, r.stderr)
        assert r.stdout == "" and not os.path.exists(tree) and not os.path.exists(log), args


def test_runs_without_the_flags_have_no_search(exe, fams, tmp_path):
    """No key of the search among the stats and no log; what such a run computes stays pinned by tests/test_cpu_mltree.py,
    tests/test_cpu_mlgamma.py and tests/test_cpu_mlancestral.py, which run unchanged."""
    r = run_s(exe, fams["aa8"], tmp_path, "plain")
    assert not any(k.startswith("ml_search") or k.startswith("ml_nni") for k in r.stats) and r.log is None


@pytest.mark.parametrize("opts", [[], ["--ml_gamma", "4"]])
def test_start_tree_reproduces_the_run(exe, fams, tmp_path, opts):
    """--ml_start with the run's own --ml_tree output: the same topology, lengths rounded to six digits, so ml_lnl within the six-digit
    bound of tests/test_cpu_mltree.py (sum over the edges of |dlnL/dt| 5e-6 t is far below 1e-3 at an optimum; asserted: 1e-6
    relative), and the same shape."""
    first = run_s(exe, fams["aa8"], tmp_path, "first", opts)
    st = write(tmp_path / "own.nwk", first.tree.strip())
    second = run_s(exe, fams["aa8"], tmp_path, "second", opts, start=st)
    assert R.shape_of(second.tree) == R.shape_of(first.tree)
    assert abs(second.stats["ml_lnl"] - first.stats["ml_lnl"]) <= 1e-6 * abs(first.stats["ml_lnl"])
    assert second.stdout == first.stdout and "ml_search_s" not in second.stats


def check_log(r, lnl_scale=1e-9):
    """Search check 2: the log's lines hang together, and where one move was applied the gain of the ratios is the difference of two
    full evaluations."""
    assert r.log and [int(line[0]) for line in r.log] == list(range(1, len(r.log) + 1))
    rows = [(int(l[1]), int(l[2]), int(l[3])) + tuple(float(x) for x in l[4:]) for l in r.log]
    assert all(len(l) == 8 for l in r.log)
    for k, (cands, positive, applied, best, before, mid, after) in enumerate(rows):
        assert before <= mid <= after, r.log[k]
        assert 0 <= applied <= positive <= cands
        if k + 1 < len(rows):
            assert after == rows[k + 1][4] and applied >= 1
        if applied == 1:
            assert abs((mid - before) - best) <= lnl_scale * abs(before), r.log[k]
        if applied == 0:
            assert before == mid == after
    assert rows[-1][6] == r.stats["ml_lnl"]
    assert r.stats["ml_search_rounds"] == sum(1 for row in rows if row[2] > 0) and r.stats["ml_nni_applied"] == sum(row[2] for row in rows)
    assert r.stats["ml_nni_calls"] == len(rows) and r.stats["ml_search_s"] > 0
    return rows


def test_start_trees_are_what_their_names_say():
    """ONE_AWAY is one of the 12 rooted NNI neighbours of the generating tree and TWO_AWAY a neighbour of that one, by a candidate
    that shares no node with the first; the splits that differ from the generating tree's are 1, 2, 2 and 4."""
    names, parent, lengths = R.from_newick(TRUE8)
    first = [x for x in N.neighbours(names, parent, lengths) if N.bipartitions(x) == N.bipartitions(ONE_AWAY)]
    assert len(first) == 1 and R.shape_of(first[0]) == R.shape_of(ONE_AWAY)
    names, parent, lengths = R.from_newick(ONE_AWAY)
    assert any(R.shape_of(x) == R.shape_of(TWO_AWAY) for x in N.neighbours(names, parent, lengths))
    assert not any(N.bipartitions(x) == N.bipartitions(SWAPPED_PAIR) for x in N.neighbours(*R.from_newick(TRUE8)))
    for text, differ in STARTS.values():
        assert len(N.bipartitions(TRUE8) - N.bipartitions(text)) == len(N.bipartitions(text) - N.bipartitions(TRUE8)) == differ


@pytest.mark.parametrize("start", list(STARTS))
def test_search_finds_the_generating_tree(exe, fams, tmp_path, start):
    """Search check 1: 8 taxa x 2000 nucleotide columns simulated on a fixed tree with inner branches 0.1 .. 0.3 (seed 1, verified on
    the CPU; seeds 2 and 3 give the same rounds and moves).  From one NNI away the search takes that one move in its first round;
    from two NNIs on edges that share no node it takes both in one round; each time the second round finds no candidate and the
    searched tree has the generating tree's bipartitions.  The two harder starts (t2 and t3 exchanged: both splits of a clade of four
    are wrong, two interchanges around adjacent edges at the least) come back too, in 3 rounds of 1 and of 2 moves: the optimiser has
    driven the edge between the wrong pairs to the lower bound, so the three resolutions around it score within 1e-2 of each other
    and the search passes through the third."""
    differ = STARTS[start][1]
    assert len(N.bipartitions(TRUE8) - N.bipartitions(open(fams[start]).read())) == differ
    r = run_s(exe, fams["sim8"], tmp_path, start, DNA(fams), search=10, start=fams[start])
    assert N.bipartitions(r.tree) == N.bipartitions(TRUE8)
    rows = check_log(r)
    applied = [row[2] for row in rows]
    print(start, "moves per round:", applied)
    assert applied[-1] == 0
    if start == "one":
        assert applied == [1, 0]
    elif start == "two":
        assert applied == [2, 0]   # both moves picked together: they share no node
    else:
        assert sum(applied) >= differ
    true = run_s(exe, fams["sim8"], tmp_path, start + "true", DNA(fams), start=fams["true"])
    assert abs(r.stats["ml_lnl"] - true.stats["ml_lnl"]) < 1.0   # (the same unrooted tree; the root may sit elsewhere)
    assert r.stats["ml_lnl_start"] < r.stats["ml_lnl"] - 100


def local_optimum(exe, fa, d, opts, index):
    """Search check 3.  The start: neighbour `index` of the plain run's tree; then every rooted NNI neighbour of the searched tree is
    optimised on its own (--ml_start, no search).  Returns the gaps lnL(searched) - lnL(neighbour), ascending."""
    plain = run_s(exe, fa, d, "plain", opts)
    names, parent, lengths = R.from_newick(plain.tree)
    st = write(os.path.join(str(d), "start.nwk"), N.neighbours(names, parent, lengths)[index])
    found = run_s(exe, fa, d, "found", opts, search=20, start=st)
    check_log(found)
    assert found.stats["ml_nni_applied"] >= 1
    names, parent, lengths = R.from_newick(found.tree)
    gaps = []
    for k, text in enumerate(N.neighbours(names, parent, lengths)):
        q = run_s(exe, fa, d, "nb%d" % k, opts, start=write(os.path.join(str(d), "nb.nwk"), text))
        gaps.append(found.stats["ml_lnl"] - q.stats["ml_lnl"])
    return sorted(gaps)


def test_searched_tree_is_a_local_optimum_amino_acids(exe, fams, tmp_path):
    """5 simulated taxa x 300 amino-acid columns: each of the 6 rooted NNI neighbours of the searched tree, its lengths optimised, has
    a lower lnL, by 100 x --ml_epsilon at the least.  Measured on the CPU: the smallest gap 0.377 (3770 x --ml_epsilon), the largest 10.46."""
    gaps = local_optimum(exe, fams["sim5"], tmp_path, [], 2)
    print("gaps:", gaps)
    assert len(gaps) == 6 and gaps[0] >= 100 * EPSILON


def test_searched_tree_is_a_local_optimum_dna_custom_model(exe, fams, tmp_path):
    """6 simulated taxa x 1000 nucleotide columns under --dna --custom_model: the 8 neighbours.  Measured on the CPU: the smallest gap
    0.513 (5130 x --ml_epsilon), the largest 46.8."""
    gaps = local_optimum(exe, fams["sim6"], tmp_path, DNA(fams), 0)
    print("gaps:", gaps)
    assert len(gaps) == 8 and gaps[0] >= 100 * EPSILON


def test_search_with_gamma_ancestral_and_one_round(exe, fams, tmp_path):
    """--ml_gamma 4 with the search, --ml_ancestral on the searched tree, --ml_search 1, -T: the files describe the searched tree."""
    opts = DNA(fams) + ["--ml_gamma", "4"]
    r = TA.run_a(exe, fams["sim8"], tmp_path, "g", ["-i", "0", "--ml_search", "10", "--ml_start", fams["swapped_pairs"], "--ml_search_log", str(tmp_path / "g.log")] + opts)
    assert N.bipartitions(r.tree) == N.bipartitions(TRUE8)
    r.log = [line.split("\t") for line in open(str(tmp_path / "g.log")).read().splitlines()]
    check_log(r)
    assert r.stats["ml_categories"] == 4 and r.rates.startswith("alpha\t")
    names, parent, lengths, labels = TA.labelled_newick(r.anctree)
    assert N.bipartitions(T_strip(r.anctree)) == N.bipartitions(TRUE8)
    assert len(TM.parse_fasta(r.anc)) == len(parent) - len(names) == 7
    assert r.sites.splitlines()[0] == "lnL %.17g" % r.stats["ml_lnl"]
    # one round from a start that needs three: never more than one round is made
    one = run_s(exe, fams["sim8"], tmp_path, "one", DNA(fams), search=1, start=fams["swapped_pairs"])
    rows = check_log(one)
    assert len(rows) == 1 and one.stats["ml_search_rounds"] <= 1
    assert one.stats["ml_lnl"] >= one.stats["ml_lnl_start"]
    # -T: what is printed stays the guide tree, the files are the search's
    t = run_s(exe, fams["sim8"], tmp_path, "t", DNA(fams) + ["-T"], search=10, start=fams["one"])
    plain_t = bu.run(exe, ["--fasta", "-i", "0", "-T"] + DNA(fams) + [fams["sim8"]])
    assert t.stdout == plain_t.stdout and N.bipartitions(t.tree) == N.bipartitions(TRUE8)
    full = run_s(exe, fams["sim8"], tmp_path, "full", DNA(fams), search=10, start=fams["one"])
    assert (t.tree, t.sites, t.log_text) == (full.tree, full.sites, full.log_text)


def T_strip(text):
    """A newick line without the labels of its inner nodes."""
    import re
    return re.sub(r"\)[^():,;]+", ")", text.strip())


def test_host_switches_do_not_change_the_oracle_driver(exe, fams, tmp_path):
    base = run_s(exe, fams["sim8"], tmp_path, "base", DNA(fams), search=10, start=fams["swapped_pairs"])
    for switch in ("PGM_HOST_TREELIK", "PGM_DEVICE_TREELIK"):   # (this driver's backend has the default body: the host loop either way)
        r = run_s(exe, fams["sim8"], tmp_path, switch, DNA(fams), search=10, start=fams["swapped_pairs"], env=dict(os.environ, **{switch: "1"}))
        assert (r.tree, r.sites, r.log_text) == (base.tree, base.sites, base.log_text)
        assert r.stats["ml_nni_kernel_ms"] == 0
