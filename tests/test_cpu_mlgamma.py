"""`--ml_gamma`, `--ml_alpha` and `--ml_rates` through the CPU oracle driver (pgmsa_oracle: Backend::tree_likelihood_rates's default, the
host loop), and the pieces below it:
  - tests/treelik_rates_ref.py itself against brute force on a 4-leaf tree (scipy's expm per category, a sum over the inner states),
    and against treelik_ref with one category;
  - tree_likelihood_rates_host and gamma_rates in a stand-alone program (tests/native/treelik_rates_test.cpp), its %a output equal to
    the statement bit for bit, the rates against scipy; built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, every other output unchanged, the three files against the statement on the written tree, the written alpha
    and the written FASTA, monotonicity, the alphabets, and the optimum against scipy's L-BFGS-B on the statement's lnL."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import gen
import mldist_general_ref as M
import test_cpu_mltree as TM
import test_cpu_treelik_shapes as SH
import treelik_rates_ref as G
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA_MIN, ALPHA_MAX = 0.05, 100.0
# gamma_rates of the host against scipy over GAMMA_GRID: the largest relative difference measured on the CPU was 7.31e-13 (alpha 100,
# K 16: the differences of I(alpha + 1, .) between neighbouring cut points are small against the values; alpha <= 2 stays below 2.2e-14).
# The test asserts ten times the measured value.
GAMMA_GRID = [(a, K) for a in (0.05, 0.1, 0.5, 1.0, 2.0, 10.0, 100.0) for K in (2, 4, 8, 16)]
GAMMA_BOUND = 7.31e-12


# ---- the statement against brute force and against the statement without categories ----------------------------------------------------
@pytest.mark.parametrize("dim", [4, 20])
def test_reference_against_brute_force(dim):
    """K = 3 categories of unequal weights.  site_l within 1e-10 relative of sum_c w_c L_c(brute force, Q r_c); d1 and d2 within 1e-5
    (relative to max(1, |value|)) of the central differences of the brute-force lnL at step 1e-4; post sums to 1 within 1e-12."""
    rng = np.random.default_rng(dim)
    Q = M.random_generator(dim, 40 + dim)   # (not reversible)
    pi = rng.dirichlet(np.ones(dim) * 3)
    parent = R.balanced(4)
    lengths = rng.uniform(0.05, 0.6, 6)
    rows = rng.integers(0, dim, (4, 12)).astype(np.int8)
    rows[1, 2] = -1; rows[:, 5] = -1; rows[3, 7] = -2
    rates, w = np.array([0.2, 0.9, 2.6]), np.array([0.3, 0.5, 0.2])
    got = G.evaluate(dim, 4, parent, rows, pi, w, G.matrices(Q, lengths, rates))
    brute = lambda t: sum(w[c] * TM.brute_site_l(Q * rates[c], pi, t, rows) for c in range(3))
    want = brute(lengths)
    assert np.all(got["site_k"] == 0)
    assert np.max(np.abs(got["site_l"] - want) / want) < 1e-10
    assert np.max(np.abs(got["post"].sum(axis=0) - 1.0)) < 1e-12 and np.all(got["post"] > 0)
    assert np.max(np.abs(got["post"][:, 5] - w)) < 1e-12   # (a column of gaps: the weights)
    lnl = lambda t: float(np.sum(np.log(brute(t))))
    step = 1e-4
    for e in range(6):
        up, dn = lengths.copy(), lengths.copy()
        up[e] += step; dn[e] -= step
        fd1 = (lnl(up) - lnl(dn)) / (2 * step)
        fd2 = (lnl(up) - 2 * lnl(lengths) + lnl(dn)) / (step * step)
        print("edge %d: d1 %.9g (differences %.9g), d2 %.9g (%.9g)" % (e, got["d1"][e], fd1, got["d2"][e], fd2))
        assert abs(got["d1"][e] - fd1) <= 1e-5 * max(1.0, abs(fd1))
        assert abs(got["d2"][e] - fd2) <= 1e-5 * max(1.0, abs(fd2))


@pytest.mark.parametrize("key", [(20, 33, "balanced8"), (4, 17, "caterpillar96"), (61, 15, "trifurcating")])
def test_one_category_is_the_old_statement(key):
    old, new = R.make_case(*key)["want"], G.make_case(*key, 1)["want"]
    for k in ("site_l", "site_k", "d1", "d2", "g", "h"):
        assert R.same_bits(new[k], old[k]), k
    assert np.all(new["post"] == 1.0)


def test_mixed_scaling_cases_hold_what_they_claim():
    c = G.make_mixed_scaling_case(4)
    assert np.any(c["diff"][c["full"]] >= 1)
    for dim in (4, 20):
        c = G.make_mixed_scaling_case(dim, 1e-6, 5)
        assert np.any(c["diff"][c["full"]] >= 5) and not np.any(np.isnan(c["want"]["d1"]))


# ---- the host loop and the rates, stand-alone ---------------------------------------------------------------------------------------------
NATIVE_CASES = [(4, n, "balanced8", k) for n in (1, 16, 17, 33) for k in (1, 2, 4)] + [(20, 33, "balanced8", 16), (64, 17, "balanced8", 2), (61, 33, "balanced8", 4),
                                                                                      (4, 33, "two", 4), (20, 33, "three", 4), (61, 15, "trifurcating", 4),
                                                                                      (20, 33, "balanced24", 4), (4, 17, "caterpillar96", 2)] + \
    SH.NATIVE_RATES   # (tests/test_cpu_treelik_shapes.py: the other dims, more than 1024 columns, polytomies)


def _case_text(c, **kw):
    d = dict(c); d.update(kw)
    nnodes = d.get("nnodes", len(d["parent"]))
    return "%d %d %d %d %d %d\n%s\n%s\n%s\n%s\n%s\n" % (d["dim"], d["nleaves"], nnodes, d["rows"].shape[1], 1 if d["derivs"] else 0, d["ncat"],
                                                    " ".join(str(int(p)) for p in d["parent"]), " ".join(str(int(v)) for v in d["rows"].reshape(-1)),
                                                    TM._hex(d["pi"]), TM._hex(d["w"]), TM._hex(d["P"]))


def _bad_cases():
    """What tree_likelihood_rates_host refuses, each a change to one small valid case: the new arguments, then what the entry without
    categories refuses."""
    c = G.make_case(4, 15, "balanced8", 2)
    bad = []
    for ncat in (0, 17):
        bad.append(_case_text(c, ncat=ncat, w=np.full(ncat, 0.5), P=np.tile(c["P"][:len(c["P"]) // 2], ncat)))
    for v in (0.0, -0.5, float("nan"), float("inf")):
        bad.append(_case_text(c, w=np.array([0.5, v])))
    old = TM._bad_cases()
    for b in old:
        bad.append(_case_text(c, parent=b["parent"], rows=b["rows"]))
    return bad


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases and the grid: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("rates_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_rates_test.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    cases = [G.make_case(d_, n, t, k) for d_, n, t, k in NATIVE_CASES] + [G.make_case(20, 33, "balanced8", 4, False), G.make_case(4, 33, "balanced8", 4, True, "unequal"),
                                                                         G.make_mixed_scaling_case(4), G.make_mixed_scaling_case(20, 1e-6, 5)]
    bad = _bad_cases()
    path = str(d / "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % (len(cases) + len(bad)))
        for c in cases:
            f.write(_case_text(c))
        for text in bad:
            f.write(text)
        f.write("%d\n" % len(GAMMA_GRID))
        for a, K in GAMMA_GRID:
            f.write("%s %d\n" % (float(a).hex(), K))
    # (-fno-sanitize=vptr: as tests/test_cpu_mltree.py, the unit holds Backend's virtual defaults without the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("rates_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    for name in flags:
        r = subprocess.run([str(d / ("rates_test_" + name)), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases %d pairs\n" % (len(cases) + len(bad), len(GAMMA_GRID))), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    return SimpleNamespace(cases=cases, bad=bad, lines=out)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_loop_equals_the_statement(native, build):
    lines, cases = native.lines[build], native.cases
    floats = lambda text: np.array([float.fromhex(x) for x in text.split()])
    for k, c in enumerate(cases):
        l, kk, post, d1, d2 = lines[5 * k:5 * k + 5]
        want, what = c["want"], (build, k, c["dim"], c["tree"], c["ncat"])
        assert R.same_bits(floats(l), want["site_l"]), what
        assert np.array_equal(np.array([int(x) for x in kk.split()], np.int32), want["site_k"]), what
        assert R.same_bits(floats(post).reshape(want["post"].shape), want["post"]), what
        if c["derivs"]:
            assert R.same_bits(floats(d1), want["d1"]) and R.same_bits(floats(d2), want["d2"]), what
        else:
            assert np.all(floats(d1) == -7.5) and np.all(floats(d2) == -7.5)   # untouched
    rejected = lines[5 * len(cases):5 * len(cases) + len(native.bad)]
    assert len(rejected) == len(native.bad) and all(line.startswith("rejected tree likelihood:") for line in rejected), rejected
    assert len(lines) == 5 * len(cases) + len(native.bad) + len(GAMMA_GRID) + 1


def test_gamma_rates_against_scipy(native):
    """Every rate of the grid within GAMMA_BOUND relative of scipy's (never above 1e-9), their average 1 within 1e-15 K, ascending; and
    the two builds print the same bits."""
    assert GAMMA_BOUND <= 1e-9
    first = 5 * len(native.cases) + len(native.bad)
    assert native.lines["plain"][first:-1] == native.lines["sanitized"][first:-1]
    worst = 0.0
    for (a, K), line in zip(GAMMA_GRID, native.lines["plain"][first:-1]):
        got = np.array([float.fromhex(x) for x in line.split()])
        want = G.gamma_rates(a, K)
        assert got.shape == (K,) and np.all(got > 0) and np.all(np.diff(got) > 0)
        diff = float(np.max(np.abs(got - want) / want))
        worst = max(worst, diff)
        print("alpha %g K %d: largest relative difference %.3g" % (a, K, diff))
        assert diff <= GAMMA_BOUND, (a, K, diff)
        total = 0.0
        for v in got:
            total = total + float(v)
        assert abs(total / K - 1.0) <= 1e-15 * K, (a, K)
    print("largest relative difference over the grid: %.3g" % worst)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def run_g(exe, fa, d, tag, opts=(), rates=True, env=None):
    p = os.path.join(str(d), tag + ".rates")
    r = TM.run_ml(exe, fa, d, tag, list(opts) + (["--ml_rates", p] if rates else []), env=env)
    r.rates = open(p).read() if os.path.exists(p) else None
    return r


def parse_rates(text):
    """(alpha, the categories' rates, per column (mean rate, category))."""
    lines = text.splitlines()
    assert lines[0].startswith("alpha\t")
    alpha = float(lines[0].split("\t")[1])
    rates, k = [], 1
    while k < len(lines) and lines[k].startswith("rate\t"):
        _, idx, v = lines[k].split("\t")
        assert int(idx) == k
        rates.append(float(v)); k += 1
    cols = []
    for c, line in enumerate(lines[k:]):
        col, mean, cat = line.split("\t")
        assert int(col) == c + 1
        cols.append((float(mean), int(cat)))
    return alpha, np.array(rates), cols


def check_files(run, kind, model, K):
    """`ml_lnl`, every --ml_sites line and every --ml_rates line against the statement on the written tree, the written alpha (%.17g:
    exact) and the written FASTA.  The newick's 6 digits move a length t by up to 5e-6 t (tests/test_cpu_mltree.py: check_files), so to
    first order a column's lnL moves by sum_e |g_e| 5e-6 t_e with the mixture's g, and its posterior of category c by
    post_c sum_e |g_ce - g_e| 5e-6 t_e; the bounds take twice that plus 1e-9 relative.  A column's category is compared where the
    two largest posteriors of the statement differ by more than their bounds.  Returns (want, names, parent, lengths, alpha)."""
    Q, pi = model
    names, parent, lengths = R.from_newick(run.tree)
    rows = R.rows_of(TM.parse_fasta(run.stdout), names, kind)
    alpha, rates, cols = parse_rates(run.rates)
    assert len(rates) == K and len(cols) == rows.shape[1] and ALPHA_MIN <= alpha <= ALPHA_MAX
    assert run.stats["ml_alpha"] == alpha and run.stats["ml_categories"] == K
    ref_rates = G.gamma_rates(alpha, K)
    assert np.max(np.abs(rates - ref_rates) / ref_rates) <= GAMMA_BOUND
    want = G.evaluate(len(pi), len(names), parent, rows, pi, G.weights_of(K), G.matrices(Q, lengths, ref_rates))
    ref = R.site_lnl(want["site_l"], want["site_k"])
    delta = 5e-6 * lengths
    bound = 2 * (np.abs(want["g"]) * delta[:, None]).sum(axis=0) + 1e-9 * np.abs(ref) + 1e-12
    lines = run.sites.splitlines()
    assert lines[0] == "lnL %.17g" % run.stats["ml_lnl"] and len(lines) == 1 + rows.shape[1]
    got = np.array([float(line.split("\t")[1]) for line in lines[1:]])
    assert [int(line.split("\t")[0]) for line in lines[1:]] == list(range(1, rows.shape[1] + 1))
    worst = float(np.max(np.abs(got - ref) / bound))
    total = float(lines[0].split()[1])
    assert abs(total - float(np.sum(ref))) <= float(np.sum(bound))
    assert abs(total - float(np.sum(got))) <= 1e-9 * abs(total)
    post = want["post"]
    post_bound = 2 * post * (np.abs(want["cat_g"] - want["g"][None]) * delta[None, :, None]).sum(axis=1) + 1e-9 * post + 1e-12
    mean = (post * ref_rates[:, None]).sum(axis=0)
    mean_bound = (post_bound * ref_rates[:, None]).sum(axis=0) + GAMMA_BOUND * mean
    got_mean = np.array([m for m, _ in cols])
    worst_mean = float(np.max(np.abs(got_mean - mean) / mean_bound))
    print("largest column difference over its bound: lnL %.3g, mean rate %.3g" % (worst, worst_mean))
    assert worst <= 1.0 and worst_mean <= 1.0
    compared = 0
    for s, (_, cat) in enumerate(cols):
        order = np.argsort(-post[:, s], kind="stable")
        assert 1 <= cat <= K
        if post[order[0], s] - post[order[1], s] > post_bound[order[0], s] + post_bound[order[1], s]:
            assert cat == order[0] + 1, s
            compared += 1
    assert compared >= rows.shape[1] // 2
    return want, names, parent, lengths, alpha


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlg_fams")
    all_fams = bu.aa_families(d)
    fams = {n: [f for f in all_fams if f.endswith("_n%d.fa" % n)][0] for n in (2, 5, 8, 13)}
    fams["dna"] = bu.dna_families(d)
    fams["codon"] = bu.codon_families(d)
    fams["hky"] = bu.hky_model(d)
    return fams


@pytest.fixture(scope="module")
def wag():
    return R.shipped("wag.qmat")


def test_refusals(exe, fams, tmp_path):
    fa = fams[5]
    tree, rates = str(tmp_path / "never.tree"), str(tmp_path / "never.rates")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    topo = str(tmp_path / "topo.nwk")
    with open(topo, "w") as f:
        f.write(bu.run(exe, ["-T", "-i", "0", fa]).stdout)
    ml = ["--ml_tree", tree]
    mg = ml + ["--ml_gamma", "4"]
    cases = [
        (["--ml_gamma", "4", fa], "need --ml_tree"),
        (["--ml_alpha", "0.5", fa], "need --ml_tree"),
        (["--ml_rates", rates, fa], "need --ml_tree"),
        (["--ml_gamma", "4", "--ml_alpha", "0.5", "--ml_rates", rates, fa], "need --ml_tree"),
        (ml + ["--ml_alpha", "0.5", fa], "need --ml_gamma"),
        (ml + ["--ml_rates", rates, fa], "need --ml_gamma"),
        (mg + [fams[2]], "at least 3 sequences"),
        (mg + ["--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_gamma", "4", "--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_alpha", "0.5", "--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_rates", rates, "--batch", lst], "--batch cannot be combined with --ml_tree"),
        (mg + ["-W", fa], "cannot be combined with -W"),
        (mg + ["-r", fa], "cannot be combined with -r"),
        (mg + ["--topology", topo, fa], "cannot be combined with --topology"),
        (mg + ["--ml_rounds", "0", fa], "from 1 to 10000"),
        (mg + ["--ml_epsilon", "-1", fa], "X >= 0"),
    ]
    for bad in ("0", "1", "17", "-4", "abc", "", "4.0", "4x", "1e1"):
        cases.append((ml + ["--ml_gamma", bad, "--ml_rates", rates, fa], "from 2 to 16"))
    for bad in ("0.049", "100.1", "0", "-1", "nan", "-nan", "inf", "-inf", "abc", "", "0.5x"):
        cases.append((mg + ["--ml_alpha", bad, "--ml_rates", rates, fa], "0.05 <= X <= 100"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [p for p in os.listdir(str(tmp_path)) if p.startswith("never") or p == "b.out"]
        assert left == [], (args, left)


def test_other_outputs_unchanged_and_stats(exe, fams, tmp_path, wag):
    fa = fams[8]
    plain = bu.run(exe, ["--fasta", "--stats", fa])
    old = TM.run_ml(exe, fa, tmp_path, "old")   # --ml_tree without the new flags: what it wrote before them
    TM.check_files(old, "aa", wag)
    assert "ml_categories" not in old.stats and "ml_alpha" not in old.stats
    r = run_g(exe, fa, tmp_path, "g", ["--ml_gamma", "4"])
    assert r.stdout == plain.stdout and len(r.stdout) > 0
    assert r.stats["ml_categories"] == 4 and ALPHA_MIN <= r.stats["ml_alpha"] <= ALPHA_MAX and r.stats["ml_kernel_ms"] == 0
    assert all(k in r.stats for k in TM.KEYS) and r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]
    assert (r.tree, r.sites) != (old.tree, old.sites)
    bs = lambda tag, extra: (bu.run(exe, ["--fasta", "--bootstrap", "4", "--bootstrap_out", str(tmp_path / tag)] + extra + [fa]).stdout, open(str(tmp_path / tag)).read())
    with_flags = bs("b1", ["--ml_tree", str(tmp_path / "b1.tree"), "--ml_sites", str(tmp_path / "b1.sites"), "--ml_gamma", "4", "--ml_rates", str(tmp_path / "b1.rates")])
    assert bs("b0", []) == with_flags
    assert [open(str(tmp_path / ("b1." + k))).read() for k in ("tree", "sites", "rates")] == [r.tree, r.sites, r.rates]   # independent of --bootstrap
    alone = run_g(exe, fa, tmp_path, "alone", ["--ml_gamma", "4"], rates=False)
    assert (alone.tree, alone.sites) == (r.tree, r.sites) and alone.rates is None
    again = TM.run_ml(exe, fa, tmp_path, "again")
    assert (again.tree, again.sites) == (old.tree, old.sites)
    for switch in ("PGM_HOST_TREELIK", "PGM_DEVICE_TREELIK"):   # (this driver's backend has the default body: the host loop either way)
        h = run_g(exe, fa, tmp_path, switch, ["--ml_gamma", "4"], env=dict(os.environ, **{switch: "1"}))
        assert (h.tree, h.sites, h.rates) == (r.tree, r.sites, r.rates) and switch in h.stats["switches"]


@pytest.mark.parametrize("n,opts", [(5, ["--ml_gamma", "4"]), (13, ["--ml_gamma", "3", "--ml_alpha", "0.7"]), (8, ["--ml_gamma", "16", "--ml_alpha", "2"])])
def test_files_aa(exe, fams, tmp_path, wag, n, opts):
    r = run_g(exe, fams[n], tmp_path, "f", ["-i", "0"] + opts)
    K = int(opts[1])
    _, _, _, lengths, alpha = check_files(r, "aa", wag, K)
    assert np.all(lengths >= 0.99e-6) and np.all(lengths <= 10.0)
    if "--ml_alpha" in opts:
        assert alpha == float(opts[3])
    assert r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]


def test_dna_custom_model_and_codon(exe, fams, tmp_path):
    hky = R.custom(fams["hky"], 4)
    fa = [f for f in fams["dna"] if len(R.read_fasta(f)) >= 3][0]
    r = run_g(exe, fa, tmp_path, "dna", ["--dna", "--custom_model", fams["hky"], "--ml_gamma", "4"])
    check_files(r, "dna", hky, 4)
    ecm = R.shipped("ecm.qmat")
    r = run_g(exe, fams["codon"][0], tmp_path, "cod", ["--codon", "--ml_rounds", "3", "--ml_gamma", "2"])
    check_files(r, "codon", ecm, 2)
    assert r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]


def test_estimated_alpha_is_never_below_alpha_one(exe, fams, tmp_path):
    """The first branch-length loop of the estimating run performs exactly the evaluations of `--ml_alpha 1`, and lnL never decreases
    afterwards."""
    for n in (5, 13):
        fixed = run_g(exe, fams[n], tmp_path, "fixed%d" % n, ["-i", "0", "--ml_gamma", "4", "--ml_alpha", "1"])
        est = run_g(exe, fams[n], tmp_path, "est%d" % n, ["-i", "0", "--ml_gamma", "4"])
        assert est.stats["ml_lnl_start"] == fixed.stats["ml_lnl_start"]
        assert est.stats["ml_lnl"] >= fixed.stats["ml_lnl"]
        assert est.stats["ml_evaluations"] >= fixed.stats["ml_evaluations"] + 12 and est.stats["ml_rounds"] >= fixed.stats["ml_rounds"]
        one = run_g(exe, fams[n], tmp_path, "one%d" % n, ["-i", "0", "--ml_gamma", "4", "--ml_alpha", "1", "--ml_rounds", "1"])
        assert one.stats["ml_rounds"] == 1 and one.stats["ml_lnl_start"] == fixed.stats["ml_lnl_start"]


# ---- the optimum ------------------------------------------------------------------------------------------------------------------------
def simulated_family(path, wag, seed=5, ntaxa=6, ncols=300, shape=0.5):
    """ntaxa sequences of ncols columns evolved under WAG down a seeded random tree without indels, every column at a rate of its own
    drawn from Gamma(shape, 1 / shape)."""
    from scipy.linalg import expm
    Q, pi = wag
    rng = np.random.default_rng(seed)
    site_rate = rng.gamma(shape, 1.0 / shape, ncols)
    seqs = [rng.choice(20, size=ncols, p=pi / pi.sum())]   # the root
    pool = [0]
    while len(pool) < ntaxa:   # split a random tip into two children
        tip = pool.pop(int(rng.integers(len(pool))))
        for _ in range(2):
            t = float(rng.uniform(0.08, 0.5))
            child = np.empty(ncols, np.int64)
            for s in range(ncols):
                P = np.clip(expm(Q * t * site_rate[s])[seqs[tip][s]], 0, None)
                child[s] = rng.choice(20, p=P / P.sum())
            seqs.append(child)
            pool.append(len(seqs) - 1)
    text = ["".join(R._AA[x] for x in seqs[k]) for k in pool]
    with open(path, "w") as f:
        f.write(gen.fasta([("A" + s[1:]) if s[0] == "M" else s for s in text]))


def test_optimum_against_scipy(exe, tmp_path, wag):
    """6 simulated taxa x 300 columns, K = 4, alpha estimated: --ml_epsilon 0 --ml_rounds 2000 against scipy.optimize.minimize (L-BFGS-B
    over the lengths and ln alpha, the same bounds, the same start: the BioNJ lengths and alpha = 1) on the statement's lnL.  As in
    tests/test_cpu_mltree.py the noise floor is the largest central-difference gradient entry of the statement at scipy's optimum; the
    driver's lnL may be below scipy's by the floor times the distance of the two optima, and its largest gradient entry must be
    within 100 x the floor.  Measured: lnL -3117.17108889 (scipy -3117.17108868), alpha 0.547974 (scipy 0.547934), floor 0.00112, the
    driver's largest gradient entry 0.0056."""
    from scipy.optimize import minimize
    fa = str(tmp_path / "sim.fa")
    simulated_family(fa, wag)
    Q, pi = wag
    K = 4
    r = run_g(exe, fa, tmp_path, "opt", ["-i", "0", "--ml_gamma", str(K), "--ml_epsilon", "0", "--ml_rounds", "2000"])
    assert r.stats["ml_rounds"] < 2000
    names, parent, ours_t = R.from_newick(r.tree)
    _, parent0, start = R.from_newick(bu.run(exe, ["-T", "-i", "1", fa]).stdout)
    assert np.array_equal(parent, parent0) and len(names) == 6
    rows = R.rows_of(TM.parse_fasta(r.stdout), names, "aa")
    assert rows.shape[1] >= 300
    ours = np.append(ours_t, math.log(r.stats["ml_alpha"]))
    nedges = len(start)
    lo = np.append(np.full(nedges, R.T_MIN), math.log(ALPHA_MIN))
    hi = np.append(np.full(nedges, R.T_MAX), math.log(ALPHA_MAX))

    def lnl(x, derivs=False):
        res = G.evaluate(20, 6, parent, rows, pi, G.weights_of(K), G.matrices(Q, x[:nedges], G.gamma_rates(math.exp(x[nedges]), K), derivs), derivs)
        return R.lnl_of(res["site_l"], res["site_k"]), res.get("d1")

    def gradient(x):
        """d1 of the statement for the lengths, a central difference of step 1e-4 for ln alpha."""
        value, d1 = lnl(x, True)
        up, dn = x.copy(), x.copy()
        up[nedges] = min(hi[nedges], x[nedges] + 1e-4); dn[nedges] = max(lo[nedges], x[nedges] - 1e-4)
        return value, np.append(d1, (lnl(up)[0] - lnl(dn)[0]) / (up[nedges] - dn[nedges]))

    def objective(x):
        value, grad = gradient(x)
        return -value, -grad

    x0 = np.append(np.clip(start, R.T_MIN, R.T_MAX), 0.0)
    sp = minimize(objective, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)))
    assert 0.1 < math.exp(sp.x[nedges]) < 10.0
    root_edges = [e for e in range(nedges) if int(parent[e]) == len(parent) - 1]

    def entries(x, grad):
        """|gradient| per free parameter: those not at a bound; the root edges (a bifurcating root) as one."""
        free = lambda e: lo[e] + 0.01 * abs(lo[e]) < x[e] < hi[e] - 0.01 * abs(hi[e])
        out = [abs(grad[e]) for e in range(len(x)) if e not in root_edges and free(e)]
        if len(root_edges) == 2:
            g = [grad[e] for e in root_edges if free(e)]
            out += [abs(sum(g) / len(g))] if g else []
        else:
            out += [abs(grad[e]) for e in root_edges if free(e)]
        return max(out) if out else 0.0

    step = 1e-4
    cd = np.zeros(len(x0))
    for e in range(len(x0)):
        up, dn = sp.x.copy(), sp.x.copy()
        up[e] = min(hi[e], up[e] + step); dn[e] = max(lo[e], dn[e] - step)
        cd[e] = (lnl(up)[0] - lnl(dn)[0]) / (up[e] - dn[e])
    floor = entries(sp.x, cd)
    ours_lnl, ours_grad = gradient(ours)
    mine = entries(ours, ours_grad)
    allowed = floor * float(np.abs(ours - sp.x).sum()) + 1e-9 * abs(sp.fun)
    print("lnL driver %.12g (statement on the written tree %.12g), scipy %.12g; alpha driver %.6g, scipy %.6g; noise floor %.3g, driver's largest gradient entry %.3g, "
          "allowed deficit %.3g" % (r.stats["ml_lnl"], ours_lnl, -sp.fun, r.stats["ml_alpha"], math.exp(sp.x[nedges]), floor, mine, allowed))
    assert floor > 0
    assert r.stats["ml_lnl"] >= -sp.fun - allowed
    assert mine <= 100 * floor
