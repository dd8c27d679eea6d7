"""`--ml_nni_opt` through the CPU oracle driver (pgmsa_oracle: Backend::tree_nni_edge's default, the host loop), and the pieces below it:
  - tests/treelik_nni_edge_ref.py itself against brute force: every candidate's exchanged tree with the trial length on the edge above
    v, evaluated with derivatives by treelik_rates_ref;
  - tree_nni_edge_host and ml_nni_edge_lengths in a stand-alone program (tests/native/treelik_nni_edge_test.cpp), its %a output equal
    to the statement bit for bit; built once plainly and once under AddressSanitizer and UBSan;
  - the optimiser's statement on the simulated 8-taxon family against a scan of the exchanged trees' lnL over the central length;
  - the driver: refusals, runs without the flag, the search and the support with it."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import test_cpu_mlsearch as TS
import test_cpu_mlsupport as TSUP
import treelik_nni_edge_ref as E
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = TS.STEP
ROUNDS = 10   # the N of --ml_nni_opt the measurements of DESIGN 3.22 were made with

# Ten times the largest deviations measured over the cases of test_statement_against_brute_force and of the caterpillar (DESIGN 3.22:
# d1 3.7e-16 of sum_s |g_s|, d2 3.2e-15 of sum_s |h_s|, the latter on the caterpillar): the two sides add the same terms in another
# association.
D1_TOL, D2_TOL = 3.7e-15, 3.2e-14
# Ten times the largest gap measured between gain_opt at N = 10 and the maximum of the scan on the 8-taxon family, in units of |lnL|
# (1.1e-16, the rounding of the sums: ten rounds reach the maximum)
SCAN_GAP = 1.1e-15


# ---- the statement against brute force ---------------------------------------------------------------------------------------------------
def brute(case, q, Z):
    """The exchanged tree of candidate q, renumbered, every edge with the matrices of the node it hangs below and the edge above v with
    the three matrices Z[k] (ncat x 3 x dim * dim) of its own, evaluated with derivatives by treelik_rates_ref.  Returns the result
    and the new number of v.  (P' and P'' of the other edges are zeros: their derivatives are not read.)"""
    dim, nleaves, parent, ncat = case["dim"], case["nleaves"], case["parent"], case["ncat"]
    nedges = len(parent) - 1
    v, a, c = (int(x) for x in case["cand"][q])
    parent2, old = N.exchanged(nleaves, parent, v, a, c)
    P = np.asarray(case["P"]).reshape(ncat, nedges, dim * dim)
    P2 = np.zeros((ncat, nedges, 3, dim * dim))
    P2[:, :, 0, :] = P[:, old[:nedges], :]
    at = int(np.where(old == v)[0][0])
    P2[:, at, :, :] = np.asarray(Z).reshape(ncat, 3, dim * dim)
    return G.evaluate(dim, nleaves, parent2, case["rows"], case["pi"], case["w"], P2.reshape(-1), derivs=True), at


def deviations(case, want, Pc, log_space=False):
    """Over every candidate: the largest relative difference of rho (or difference of log rho) and of d1, d2 relative to sum |g|, sum |h|."""
    dim, ncat, ncand = case["dim"], case["ncat"], len(case["cand"])
    Z = np.asarray(Pc).reshape(ncat, ncand, 3 * dim * dim)
    here = want
    worst = [0.0, 0.0, 0.0]
    for q in range(ncand):
        there, at = brute(case, q, Z[:, q])
        if log_space:
            with np.errstate(divide="ignore"):
                ratio = (np.log(there["site_l"]) - STEP * there["site_k"]) - (np.log(here["site_l"]) - STEP * here["site_k"])
            worst[0] = max(worst[0], float(np.max(np.abs(np.log(want["rho"][q]) - ratio))))
        else:
            assert np.all(there["site_k"] == 0) and np.all(here["site_k"] == 0)
            ratio = there["site_l"] / here["site_l"]
            worst[0] = max(worst[0], float(np.max(np.abs(want["rho"][q] - ratio) / ratio)))
        worst[1] = max(worst[1], abs(want["d1"][q] - there["d1"][at]) / float(np.sum(np.abs(there["g"][at]))))
        worst[2] = max(worst[2], abs(want["d2"][q] - there["d2"][at]) / float(np.sum(np.abs(there["h"][at]))))
    return worst


def generator_edge_case(dim, tree, ncat, seed):
    """test_cpu_mlsearch.generator_case (a generator that is not reversible, columns with gaps and -2) and per candidate a trial length:
    the tree's own, both bounds and random ones in turn."""
    import mldist_general_ref as M
    case = TS.generator_case(dim, tree, ncat, seed)
    nedges = len(case["parent"]) - 1
    rng = np.random.default_rng(seed)   # (generator_case's own draws of pi and the lengths, restated: checked against its P below)
    rng.dirichlet(np.ones(dim) * 3)
    lengths = rng.uniform(0.05, 0.6, nedges)
    Q = M.random_generator(dim, 40 + dim)
    rates = np.array([1.0]) if ncat == 1 else np.array([0.2, 0.7, 1.1, 2.0])
    assert R.same_bits(G.matrices(Q, lengths, rates, derivs=False), case["P"])
    trng = np.random.default_rng(seed + 1)
    t = []
    for q, (v, _, _) in enumerate(case["cand"]):
        t.append([lengths[int(v)], E.T_MIN, E.T_MAX, float(trng.uniform(0.01, 2.0))][q % 4])
    Pc = G.matrices(Q, t, rates, derivs=True)
    return dict(case, Pc=Pc, t=t, lengths=lengths, want=E.evaluate(dim, case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], case["cand"], Pc),
                nni_want=case["want"])


@pytest.mark.parametrize("dim,tree,ncat", TS.BRUTE)
def test_statement_against_brute_force(dim, tree, ncat):
    """Every candidate of the balanced tree of 8, of the trifurcating root and of the inner trifurcation under a generator that is not
    reversible: rho within 1e-10 relative of the ratio of the two trees' site likelihoods (DESIGN 3.20's bound), d1 and d2 within
    D1_TOL and D2_TOL of that edge's derivatives in the exchanged tree."""
    case = generator_edge_case(dim, tree, ncat, 300 + dim + ncat + sum(map(ord, tree)))
    worst = deviations(case, case["want"], case["Pc"])
    print("largest deviations: rho %.3g, d1 %.3g, d2 %.3g" % tuple(worst))
    assert worst[0] < 1e-10 and worst[1] < D1_TOL and worst[2] < D2_TOL
    own = [q for q in range(len(case["cand"])) if q % 4 == 0]   # at the tree's own length rho is the plain statement's
    assert R.same_bits(case["want"]["rho"][own], case["nni_want"]["rho"][own])


def test_caterpillar_scaling_in_log_space():
    """The caterpillar of 96 leaves: some candidate has k_N != k_D on some column; there log rho is within 1e-10 of the brute-force log
    ratio and d1, d2 within the same bounds."""
    case = E.make_case(4, 17, "caterpillar96", 1)
    nw = case["nni_want"]
    differs = np.argwhere((nw["cat_kd"][0] != nw["cat_kn"][0]).any(axis=1))[:, 0]
    assert len(differs) > 0
    pick = [int(q) for q in list(differs[:4]) + list(differs[-4:])]
    sub = dict(case, cand=case["cand"][pick])
    Pc = np.asarray(case["Pc"]).reshape(1, len(case["cand"]), -1)[:, pick]
    want = {k: (v[pick] if k in ("rho", "d1", "d2", "g", "h") else v) for k, v in case["want"].items()}
    worst = deviations(sub, want, Pc.reshape(-1), log_space=True)
    print("largest deviations: log rho %.3g, d1 %.3g, d2 %.3g" % tuple(worst))
    assert worst[0] < 1e-10 and worst[1] < D1_TOL and worst[2] < D2_TOL


def test_zeros_and_own_blocks():
    """D == 0 and rho == 0 both occur with g = h = 0 (asserted where the case is made); Pc = P_v reproduces treelik_nni_ref's rho bit for
    bit; one category with w = {1.0}: the site values are the plain statement's."""
    E.zeros_case()
    for key in [(4, 33, "balanced8", 4), (20, 17, "inner3", 2), (4, 17, "caterpillar96", 1), (61, 15, "balanced8", 1)]:
        c = E.make_case(*key, own=True)
        assert R.same_bits(c["want"]["rho"], c["nni_want"]["rho"]), key
        for k in ("site_l", "site_k", "post"):
            assert R.same_bits(c["want"][k], c["nni_want"][k]), (key, k)
    c = E.make_case(61, 15, "balanced8", 1)
    plain = R.evaluate(61, c["nleaves"], c["parent"], c["rows"], c["pi"], c["P"], derivs=False)
    assert c["w"].tolist() == [1.0] and R.same_bits(c["want"]["site_l"], plain["site_l"]) and np.array_equal(c["want"]["site_k"], plain["site_k"])


# ---- the host code, stand-alone ----------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_mlnniopt.py, which takes these lists from here: the host loop runs every one of them.
GRID = TS.GRID
# (spb = 64 / dim sites per wavefront, four wavefronts per workgroup of the candidates' kernel: both edges of both)
OTHER_DIMS = [(dim, ncols, "balanced8", 2) for dim in (1, 2, 3, 5, 33, 63) for ncols in sorted({1, 64 // dim, 64 // dim + 1, 4 * (64 // dim), 4 * (64 // dim) + 1})]
TREES = TS.SMALL_TREES + TS.ARITY + TS.LARGER
ORDER = TS.ORDER
LONG = [(4, 1025, "three", 2)]   # 65 chunks of sites: the second round of the sums kernel's chunk loop
SMALL_VALID = TS.SMALL_VALID


def same_candidate_case():
    """One candidate eight times, each time with other matrices (other trial lengths)."""
    base = N.make_case(20, 17, "balanced8", 2)
    nb = dict(base, cand=np.ascontiguousarray(base["cand"][[5] * 8]))
    nb["want"] = N.evaluate(20, 8, base["parent"], base["rows"], base["pi"], base["w"], base["P"], nb["cand"])
    return E.with_pc(nb, E.draw_pc(np.random.default_rng(31), 2, 8, 20, "balanced8"), tree="balanced8, one candidate eight times")


def leaf_case():
    base = TS.leaf_case()
    return E.with_pc(base, E.draw_pc(np.random.default_rng(32), 2, len(base["cand"]), 4, "leaves"))


def many_candidates_case():
    """70001 candidates x dim 2 x one column: the two candidates of the tree of 3 leaves in turn, each with one of five sets of matrices
    (so the expectation is that of ten pairs, repeated)."""
    base = N.make_case(2, 1, "three", 2)
    pc10 = E.draw_pc(np.random.default_rng(33), 2, 10, 2, "three").reshape(2, 10, 12)
    ten = dict(base, cand=np.ascontiguousarray(base["cand"][np.arange(10) % 2]))
    ten["want"] = N.evaluate(2, 3, base["parent"], base["rows"], base["pi"], base["w"], base["P"], ten["cand"])
    ten = E.with_pc(ten, pc10.reshape(-1))
    pick = np.arange(70001) % 10
    want = dict(ten["want"])
    for k in ("rho", "g", "h", "d1", "d2"):
        want[k] = np.ascontiguousarray(ten["want"][k][pick])
    return dict(ten, cand=np.ascontiguousarray(ten["cand"][pick]), Pc=np.ascontiguousarray(pc10[:, pick]).reshape(-1), want=want, tree="three, 70001 candidates")


_extra = {}


def extra_cases():
    if not _extra:
        _extra.update(same=same_candidate_case(), leaves=leaf_case(), many=many_candidates_case(), zeros=E.zeros_case())
    return _extra


def all_keys():
    return list(dict.fromkeys(GRID + OTHER_DIMS + TREES + ORDER + LONG + [SMALL_VALID]))


def optimiser_case(key, seed, rounds=ROUNDS):
    """A case of the optimiser over the rational family of matrices: lengths drawn, the tree's own P of the family at them."""
    base = N.make_case(*key)
    dim, ncat, nedges = base["dim"], base["ncat"], len(base["parent"]) - 1
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.01, 1.0, (ncat, dim, dim)); A /= A.sum(axis=2, keepdims=True)
    B = rng.uniform(0.01, 1.0, (ncat, dim, dim)); B /= B.sum(axis=2, keepdims=True)
    lengths = rng.uniform(0.02, 0.8, nedges)
    fam = E.rational_matrices(A, B)
    own = np.asarray(fam(list(lengths))).reshape(ncat, nedges, 3, dim * dim)
    P = np.ascontiguousarray(own[:, :, 0, :]).reshape(-1)
    case = dict(base, P=P, A=A, B=B, lengths=lengths, rounds=rounds)
    case["nni_rho"] = N.evaluate(dim, base["nleaves"], base["parent"], base["rows"], base["pi"], base["w"], P, base["cand"])["rho"]
    case["opt"] = E.optimise(case, fam, lengths, rounds)
    return case


OPT_KEYS = [((4, 33, "balanced8", 4), 1), ((20, 17, "inner3", 2), 2), ((4, 17, "balanced8", 1), 3), ((61, 15, "trifurcating", 2), 4)]


def _case_bytes(c, rounds=0, null=0, **kw):
    d = dict(c); d.update(kw)
    cand = np.asarray(d["cand"], np.uint32).reshape(-1, 3)
    head = np.array([d["dim"], d["nleaves"], d.get("nnodes", len(d["parent"])), d["rows"].shape[1], d["ncat"], d.get("ncand", len(cand)), rounds, null], np.int32)
    parts = [head, np.asarray(d["parent"], np.uint32), np.asarray(d["rows"], np.int8), np.asarray(d["pi"], np.float64), np.asarray(d["w"], np.float64), np.asarray(d["P"], np.float64), cand]
    parts += [np.asarray(d["lengths"], np.float64), R.pack(d["A"][:, None]), R.pack(d["B"][:, None])] if rounds else [np.asarray(d["Pc"], np.float64)]
    return b"".join(np.ascontiguousarray(x).tobytes() for x in parts)


def _bad_cases():
    c = E.make_case(*SMALL_VALID)
    bad = [_case_bytes(c, null=k) for k in (1, 2, 3)]
    bad.append(_case_bytes(c, cand=np.zeros((0, 3), np.uint32), Pc=np.zeros(0)))
    for cand in TS.bad_candidates():
        bad.append(_case_bytes(c, cand=np.array(cand, np.uint32), Pc=c["Pc"][:2 * len(cand) * 48]))
    for ncat in (0, 17):
        bad.append(_case_bytes(c, ncat=ncat, w=np.full(ncat, 0.5), P=np.tile(c["P"][:len(c["P"]) // 2], ncat), Pc=np.zeros(min(ncat, 64) * 12 * 48)))
    bad.append(_case_bytes(c, w=np.array([0.5, float("nan")])))
    for b in TS.TM._bad_cases():
        bad.append(_case_bytes(c, parent=b["parent"], rows=b["rows"], cand=c["cand"][:1], Pc=c["Pc"][:2 * 48]))
    return bad


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("nni_edge_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_nni_edge_test.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    cases = [E.make_case(*k) for k in all_keys()] + list(extra_cases().values())
    opts = [optimiser_case(k, seed) for k, seed in OPT_KEYS]
    bad = _bad_cases()
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases) + len(opts) + len(bad)], np.int32).tobytes())
        for c in cases:
            f.write(_case_bytes(c))
        for c in opts:
            f.write(_case_bytes(c, rounds=c["rounds"]))
        for blob in bad:
            f.write(blob)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("edge_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    total = len(cases) + len(opts) + len(bad)
    for name, args in (("plain", []), ("sanitized", []), ("plain, a block per chunk", ["1"]), ("plain, one candidate per group", ["0", "1"])):
        r = subprocess.run([str(d / ("edge_test_" + name.split(",")[0])), path] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % total), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    return SimpleNamespace(cases=cases, opts=opts, bad=bad, lines=out)


@pytest.mark.parametrize("build", ["plain", "sanitized", "plain, a block per chunk", "plain, one candidate per group"])
def test_host_code_equals_the_statement(native, build):
    lines, cases = native.lines[build], native.cases
    floats = lambda text: np.array([float.fromhex(x) for x in text.split()])
    for k, c in enumerate(cases):
        l, kk, post, rho, d1, d2 = lines[6 * k:6 * k + 6]
        want, what = c["want"], (build, k, c["dim"], c["tree"], c["ncat"])
        assert not np.any(np.isnan(want["rho"])) and not np.any(np.isnan(want["d1"])) and not np.any(np.isnan(want["d2"])), what
        assert R.same_bits(floats(l), want["site_l"]), what
        assert np.array_equal(np.array([int(x) for x in kk.split()], np.int32), want["site_k"]), what
        assert R.same_bits(floats(post).reshape(want["post"].shape), want["post"]), what
        assert R.same_bits(floats(rho).reshape(want["rho"].shape), want["rho"]), what
        assert R.same_bits(floats(d1), want["d1"]) and R.same_bits(floats(d2), want["d2"]), what
    first = 6 * len(cases)
    for k, c in enumerate(native.opts):
        t, gain, rho = lines[first + 3 * k:first + 3 * k + 3]
        t_opt, gain_opt, rows, trials = c["opt"]
        what = (build, "optimiser", k)
        assert R.same_bits(floats(t), t_opt) and R.same_bits(floats(gain), gain_opt) and R.same_bits(floats(rho).reshape(rows.shape), rows), what
    first += 3 * len(native.opts)
    rejected = lines[first:first + len(native.bad)]
    assert len(rejected) == len(native.bad) and all(line.startswith("rejected tree ") for line in rejected), rejected
    assert sum(line.startswith("rejected tree nni:") for line in rejected) == 1 + len(TS.bad_candidates())
    assert len(lines) == first + len(native.bad) + 1


@pytest.mark.parametrize("key,seed", OPT_KEYS)
def test_optimiser_statement_properties(key, seed):
    """Round 0 is the plain statement's row; gain_opt is never below the gain there; a group per candidate gives the same bits; every
    trial stays within the bounds; more rounds never lower a gain."""
    c = optimiser_case(key, seed)
    t_opt, gain_opt, rows, trials = c["opt"]
    g0 = N.gain(c["nni_rho"])
    assert np.all(gain_opt >= g0) and np.any(gain_opt > g0)
    zero = E.optimise(c, E.rational_matrices(c["A"], c["B"]), c["lengths"], 0)
    assert R.same_bits(zero[2], c["nni_rho"]) and R.same_bits(zero[1], g0) and R.same_bits(zero[0], c["lengths"][c["cand"][:, 0].astype(int)])
    assert all(E.T_MIN <= t <= E.T_MAX for trial in trials for t in trial)
    if seed == 3:
        single = E.optimise(c, E.rational_matrices(c["A"], c["B"]), c["lengths"], c["rounds"], group=1)
        assert all(R.same_bits(a, b) for a, b in zip(single[:3], c["opt"][:3]))
        fewer = E.optimise(c, E.rational_matrices(c["A"], c["B"]), c["lengths"], 3)
        assert np.all(fewer[1] <= gain_opt)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


fams = TSUP.fams
DNA = TS.DNA


def test_refusals(exe, fams, tmp_path):
    fa = fams["aa5"]
    tree, sup, log = str(tmp_path / "never.tree"), str(tmp_path / "never.sup"), str(tmp_path / "never.log")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    ml, s, se = ["--ml_tree", tree], ["--ml_support", sup], ["--ml_search", "3"]
    cases = [
        (["--ml_nni_opt", "3", fa], "--ml_nni_opt needs --ml_tree"),
        (ml + ["--ml_nni_opt", "3", fa], "--ml_nni_opt needs --ml_search or --ml_support"),
        (ml + ["--ml_nni_opt", "3", "--ml_search_log", log, fa], "--ml_search_log needs --ml_search"),
        (ml + se + ["--ml_nni_opt", "3", "-W", fa], "cannot be combined with -W"),
        (ml + se + ["--ml_nni_opt", "3", "-r", fa], "cannot be combined with -r"),
        (ml + s + ["--ml_nni_opt", "3", "--topology", fams["true"], fa], "cannot be combined with --topology"),
        (ml + se + ["--ml_nni_opt", "3", "--batch", lst], "--batch cannot be combined"),
        (ml + se + ["--ml_nni_opt", "3", "--ml_gamma", "1", fa], "--ml_gamma takes"),
        (ml + ["--ml_search", "0", "--ml_nni_opt", "3", fa], "--ml_search takes"),
        (ml + s + ["--ml_nni_opt", "3", "--ml_support_reps", "0", fa], "--ml_support_reps takes"),
        (ml + s + ["--ml_nni_opt", "3", fams["aa3"]], "--ml_support needs at least 4 sequences"),
    ]
    for text in ("0", "21", "-1", "abc", "1.5", "", "3x"):
        cases.append((ml + se + ["--ml_nni_opt", text, fa], "--ml_nni_opt takes a number of rounds from 1 to 20"))
        cases.append((ml + s + ["--ml_nni_opt", text, fa], "--ml_nni_opt takes a number of rounds from 1 to 20"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta", "-i", "0"] + args, code=2)
        assert "ERROR:" in r.stderr and message in r.stderr, (args, r.stderr)
        assert r.stdout == "" and not any(os.path.exists(p) for p in (tree, sup, log)), args


def test_runs_without_the_flag_have_no_keys_and_the_help_is_silent(exe, fams, tmp_path):
    r = TSUP.run_sup(exe, fams["sim8"], tmp_path, "plain", DNA(fams) + ["--ml_start", fams["one"], "--ml_search", "5"], reps=20)
    assert not any(k.startswith("ml_nni_opt") for k in r.stats)
    w = TSUP.run_sup(exe, fams["sim8"], tmp_path, "with", DNA(fams) + ["--ml_start", fams["one"], "--ml_search", "5", "--ml_nni_opt", "2"], reps=20)
    assert w.stats["ml_nni_opt_s"] > 0 and w.stats["ml_nni_opt_calls"] >= 3 * 3 and w.stats["ml_nni_opt_kernel_ms"] == 0
    h = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "ml_nni_opt" not in h.stdout + h.stderr


def search(exe, fams, d, tag, start, opts=(), n=ROUNDS):
    return TS.run_s(exe, fams["sim8"], d, tag, DNA(fams) + list(opts) + (["--ml_nni_opt", str(n)] if n else []), search=10, start=fams[start])


@pytest.fixture(scope="module")
def starts(fams):
    for name, (text, _) in TS.STARTS.items():
        fams[name] = TS.write(os.path.join(str(fams["dir"]), name + ".nwk"), text)
    return fams


@pytest.mark.parametrize("start,opts", [(s, []) for s in TS.STARTS] + [(s, ["--ml_gamma", "4"]) for s in ("one", "swapped_pairs")])
def test_search_with_the_option(exe, starts, tmp_path, start, opts):
    """DESIGN 3.20's simulated 8-taxon fixtures: the log hangs together (lnl_before <= lnl_applied <= lnl_after; where one move was
    applied lnl_applied - lnl_before is best_gain to 1e-9 |lnL|: the optimised gain is a full evaluation of the exchanged tree at
    t_opt), and the searched tree has the generating tree's bipartitions."""
    r = search(exe, starts, tmp_path, start, start, opts)
    rows = TS.check_log(r)
    assert N.bipartitions(r.tree) == N.bipartitions(TS.TRUE8)
    plain = search(exe, starts, tmp_path, start + "plain", start, opts, n=0)
    print(start, opts, "moves per round with the option:", [row[2] for row in rows], "without:", [int(l[3]) for l in plain.log])
    assert r.stats["ml_nni_opt_calls"] == (ROUNDS + 1) * len(rows) and r.stats["ml_nni_calls"] == len(rows)
    assert float(r.log[0][4]) >= float(plain.log[0][4])   # the first round ranks the same candidates: the best optimised gain is no lower
    assert r.stats["ml_lnl"] >= plain.stats["ml_lnl"] - 1e-6 * abs(plain.stats["ml_lnl"])


def scan_max(case, fam_of, q, lo=E.T_MIN, hi=E.T_MAX):
    """The maximum of the exchanged tree's gain over the central length: 41 lengths spaced evenly in log t, then 41 between the
    neighbours of the best, five times."""
    best = -math.inf
    for level in range(6):
        ts = list(np.exp(np.linspace(math.log(lo), math.log(hi), 41)))
        sub = dict(case, cand=case["cand"][[q] * len(ts)])
        o = E.evaluate(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], sub["cand"], fam_of(ts))
        gains = N.gain(o["rho"])
        k = int(np.argmax(gains))
        best = max(best, float(gains[k]))
        lo, hi = ts[max(k - 1, 0)], ts[min(k + 1, len(ts) - 1)]
    return best


def test_optimised_gains_against_a_scan(fams):
    """The simulated 8-taxon family on the start with t2 and t3 exchanged, lengths as written: every candidate's gain_opt at N = 10 is no
    lower than its gain at the tree's own length, no higher than the maximum of a scan of the exchanged tree's lnL over the central
    length plus 1e-9 |lnL|, and within SCAN_GAP |lnL| below it."""
    hky = R.custom(fams["hky"], 4)
    Q, pi = hky
    names, parent, lengths = R.from_newick(TS.SWAPPED_PAIR)
    seqs = R.read_fasta(fams["sim8"])
    rows = np.array(R.rows_of(seqs, names, "dna"), np.int8)
    rates, w = np.array([1.0]), np.array([1.0])
    P = G.matrices(Q, lengths, rates, derivs=False)
    cand = N.candidates(len(names), parent)
    case = dict(dim=4, nleaves=len(names), parent=parent, rows=rows, pi=pi / pi.sum(), w=w, P=P, ncat=1, cand=cand)
    fam_of = lambda ts: G.matrices(Q, ts, rates, derivs=True)
    t_opt, gain_opt, rho, trials = E.optimise(case, fam_of, lengths, ROUNDS)
    here = G.evaluate(4, case["nleaves"], parent, rows, case["pi"], w, P, derivs=False)
    lnl = abs(R.lnl_of(here["site_l"], here["site_k"]))
    g0 = N.gain(N.evaluate(4, case["nleaves"], parent, rows, case["pi"], w, P, cand)["rho"])
    assert np.all(gain_opt >= g0)
    gaps = []
    for q in range(len(cand)):
        top = scan_max(case, fam_of, q)
        assert gain_opt[q] <= top + 1e-9 * lnl, (q, gain_opt[q], top)
        gaps.append((top - gain_opt[q]) / lnl)
    print("lnL %.3f; largest gap below the scan's maximum / |lnL|: %.3g; gains gained: %s" % (-lnl, max(gaps), np.round(gain_opt - g0, 3).tolist()))
    assert max(gaps) <= SCAN_GAP


def test_support_with_the_option(exe, fams, tmp_path):
    """With the flag and without on the same run otherwise: alrt with the flag is no higher for every supported node (the round-0 row
    is the unoptimised one); hits lie within 0 .. N; the same seed gives the same files; the zero-length-branch family keeps its node
    below the cut and the others above; --ml_gamma 4, behind --ml_search and --ml_nni_opt 1 run."""
    base = DNA(fams) + ["--ml_start", fams["true"]]
    for tag, fa, extra, reps in (("t", "sim8", [], 200), ("g", "sim8", ["--ml_gamma", "4"], 50), ("s", "sim8", ["--ml_search", "5"], 50), ("z", "zero8", [], 1000)):
        start = ["--ml_start", fams["zero"]] if fa == "zero8" else ["--ml_start", fams["one"]] if "--ml_search" in extra else ["--ml_start", fams["true"]]
        opts = DNA(fams) + start + extra
        off = TSUP.run_sup(exe, fams[fa], tmp_path, tag + "off", opts, reps=reps)
        on = TSUP.run_sup(exe, fams[fa], tmp_path, tag + "on", opts + ["--ml_nni_opt", "5"], reps=reps)
        TSUP.check_shapes(on, reps, 1)
        if "--ml_search" not in extra:   # (behind the search the two runs may rank other moves)
            assert (on.tree, on.sites) == (off.tree, off.sites)
            assert [n[0] for n in on.nodes] == [n[0] for n in off.nodes]
            assert all(a[2] <= b[2] for a, b in zip(on.nodes, off.nodes)), (on.nodes, off.nodes)
        assert all(0 <= n[3] <= reps and 0 <= n[4] <= reps for n in on.nodes)
        assert on.stats["ml_nni_opt_calls"] >= 6 and on.stats["ml_support_calls"] == off.stats["ml_support_calls"]
        if tag == "t":
            again = TSUP.run_sup(exe, fams[fa], tmp_path, tag + "again", opts + ["--ml_nni_opt", "5"], reps=reps)
            assert (again.support, again.table) == (on.support, on.table)
            one = TSUP.run_sup(exe, fams[fa], tmp_path, tag + "one", opts + ["--ml_nni_opt", "1"], reps=reps)
            assert all(a[2] <= b[2] for a, b in zip(one.nodes, off.nodes)) and all(a[2] <= b[2] for a, b in zip(on.nodes, one.nodes))
            assert one.stats["ml_nni_opt_calls"] == 2
        if tag == "z":
            print(on.nodes)
            assert [n[0] for n in on.nodes] == ["N1", "N2", "N4", "N5"]
            assert on.nodes[0][3] < TSUP.CUT * reps and on.nodes[0][4] < TSUP.CUT * reps
            assert all(n[3] > TSUP.CUT * reps and n[4] > TSUP.CUT * reps for n in on.nodes[1:])
