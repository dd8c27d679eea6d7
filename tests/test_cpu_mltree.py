"""`--ml_tree`, `--ml_sites`, `--ml_rounds` and `--ml_epsilon` through the CPU oracle driver (pgmsa_oracle: Backend::tree_likelihood's
default, the host loop), and the pieces below it:
  - tests/treelik_ref.py itself against brute force on a 4-leaf tree and on a tree with an inner node of four children (scipy's expm,
    a sum over the states of the inner nodes below the root), from one state to 20;
  - tree_likelihood_host in a stand-alone program (tests/native/treelik_test.cpp), its %a output equal to treelik_ref bit for bit,
    built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, every other output unchanged, topology, the two files against treelik_ref on the written tree and the
    written FASTA, monotonicity, the alphabets, and the optimum against scipy's L-BFGS-B on treelik_ref's lnL."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import gen
import mldist_general_ref as M
import test_cpu_treelik_shapes as SH
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ml_tree_s", "ml_rounds", "ml_evaluations", "ml_lnl_start", "ml_lnl", "ml_kernel_ms")


# ---- the statement against brute force --------------------------------------------------------------------------------------------
def brute_site_l(Q, pi, lengths, rows, tree="balanced4"):
    """A sum over the states of the inner nodes below the root (einsum over explicit matrices, every index looped; scipy's expm):
    ((0,1)4,(2,3)5)6, or treelik_ref's inner4, (6,(4,5,(0,1)7,(2,3)8)9)10."""
    from scipy.linalg import expm
    P = [expm(Q * t) for t in lengths]
    n = len(pi)
    out = []
    for s in range(rows.shape[1]):
        u = [np.ones(n) if rows[l, s] < 0 else np.eye(n)[rows[l, s]] for l in range(rows.shape[0])]
        if tree == "balanced4":
            out.append(np.einsum("r,ra,a,a,rb,b,b->", pi, P[4], P[0] @ u[0], P[1] @ u[1], P[5], P[2] @ u[2], P[3] @ u[3]))
        else:
            assert tree == "inner4"
            out.append(np.einsum("r,r,rc,c,c,ca,a,a,cb,b,b->", pi, P[6] @ u[6], P[9], P[4] @ u[4], P[5] @ u[5], P[7], P[0] @ u[0], P[1] @ u[1],
                                 P[8], P[2] @ u[2], P[3] @ u[3]))
    return np.array(out)


BRUTE = [(dim, tree) for tree in ("balanced4", "inner4") for dim in (1, 3, 4, 8, 20)]


@pytest.mark.parametrize("dim,tree", BRUTE, ids=[str(dim) if tree == "balanced4" else "%d-%s" % (dim, tree) for dim, tree in BRUTE])
def test_reference_against_brute_force(dim, tree):
    """L_s within 1e-10 relative (at most 3 * 64^2 terms of one sign: rounding is far below it); d1 and d2 within 1e-5 (relative
    to max(1, |value|)) of the first and second central differences of the brute-force lnL at step 1e-4.  inner4 has a node of four
    children below the root, two of them inner: the general branch of the down pass with an outside vector behind it.  One state has
    one generator, Q = 0: every likelihood is 1 and every derivative 0."""
    rng = np.random.default_rng(dim)
    Q = M.random_generator(dim, 40 + dim) if dim > 1 else np.zeros((1, 1))   # (not reversible: the direction parent -> child matters)
    pi = rng.dirichlet(np.ones(dim) * 3)
    if tree == "balanced4":
        nleaves, parent = 4, R.balanced(4)
        assert list(parent) == [4, 4, 5, 5, 6, 6, R.ROOT]
    else:
        nleaves, parent = R.TREES["inner4"]()
        assert list(parent) == [7, 7, 8, 8, 9, 9, 10, 9, 9, 10, R.ROOT]
    nedges = len(parent) - 1
    lengths = rng.uniform(0.05, 0.6, nedges)
    rows = rng.integers(0, dim, (nleaves, 12)).astype(np.int8)
    rows[1, 2] = -1; rows[:, 5] = -1; rows[3, 7] = -2
    got = R.evaluate(dim, nleaves, parent, rows, pi, R.matrices(Q, lengths))
    want = brute_site_l(Q, pi, lengths, rows, tree)
    assert np.all(got["site_k"] == 0)
    assert np.max(np.abs(got["site_l"] - want) / want) < 1e-10
    assert abs(want[5] - 1.0) < 1e-12   # (a column of gaps)
    lnl = lambda t: float(np.sum(np.log(brute_site_l(Q, pi, t, rows, tree))))
    step = 1e-4
    for e in range(nedges):
        up, dn = lengths.copy(), lengths.copy()
        up[e] += step; dn[e] -= step
        fd1 = (lnl(up) - lnl(dn)) / (2 * step)
        fd2 = (lnl(up) - 2 * lnl(lengths) + lnl(dn)) / (step * step)
        print("edge %d: d1 %.9g (differences %.9g), d2 %.9g (%.9g)" % (e, got["d1"][e], fd1, got["d2"][e], fd2))
        assert abs(got["d1"][e] - fd1) <= 1e-5 * max(1.0, abs(fd1))
        assert abs(got["d2"][e] - fd2) <= 1e-5 * max(1.0, abs(fd2))


def test_reference_scaling_is_exact():
    """A caterpillar deep enough to rescale: the pair (site_l, site_k) is the unscaled likelihood, computed here in logarithms."""
    c = R.make_case(4, 17, "caterpillar96")
    full = (c["rows"] >= 0).all(axis=0)
    assert full.sum() >= 8 and np.all(c["want"]["site_k"][full] > 0)
    X = R.unpack(c["P"], 190, 3, 4)
    kids = R.children_of(c["parent"])
    for s in np.flatnonzero(full)[:3]:
        logu = {}
        for v in range(191):
            if v < 96:
                logu[v] = np.where(np.arange(4) == c["rows"][v, s], 0.0, -np.inf)
            else:
                acc = np.zeros(4)
                for k in kids[v]:
                    acc += np.log(X[k][0] @ np.exp(logu[k] - logu[k].max())) + logu[k].max()
                logu[v] = acc
        want = np.log(np.sum(c["pi"] * np.exp(logu[190] - logu[190].max()))) + logu[190].max()
        got = R.site_lnl(c["want"]["site_l"], c["want"]["site_k"])[s]
        assert abs(got - want) < 1e-9 * abs(want)


# ---- the host loop, bit for bit -------------------------------------------------------------------------------------------------------
NATIVE_CASES = [(4, n, "balanced8", True) for n in (1, 15, 16, 17, 33, 300)] + [(20, n, "balanced8", True) for n in (1, 16, 17, 33)] + \
    [(64, 17, "balanced8", True), (61, 33, "balanced8", True), (4, 33, "two", True), (20, 33, "three", True), (61, 15, "trifurcating", True), (4, 33, "trifurcating", True),
     (20, 33, "balanced24", True), (4, 17, "caterpillar96", True), (20, 17, "caterpillar96", True), (20, 33, "balanced8", False), (4, 17, "caterpillar96", False)] + \
    SH.NATIVE_PLAIN   # (tests/test_cpu_treelik_shapes.py: the other dims, more than 1024 columns, polytomies)


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _case_text(dim, nleaves, parent, rows, pi, P, derivs):
    return "%d %d %d %d %d\n%s\n%s\n%s\n%s\n" % (dim, nleaves, len(parent), rows.shape[1], 1 if derivs else 0, " ".join(str(int(p)) for p in parent),
                                                " ".join(str(int(v)) for v in rows.reshape(-1)), _hex(pi), _hex(P))


def _bad_cases():
    """What tree_likelihood_host refuses, each a change to one small valid case."""
    c = R.make_case(4, 15, "balanced8")
    base = dict(dim=4, nleaves=8, parent=c["parent"].copy(), rows=c["rows"].copy(), pi=c["pi"], P=c["P"], derivs=True)
    bad = []
    def variant(**kw):
        d = dict(base); d.update(kw); bad.append(d)
    p = base["parent"].copy(); p[8] = 8; variant(parent=p)                    # a parent index <= its child
    p = base["parent"].copy(); p[0] = 3; variant(parent=p)                    # a leaf that is a parent
    p = base["parent"].copy(); p[13] = R.ROOT; variant(parent=p)              # two roots
    p = base["parent"].copy(); p[0] = 9; variant(parent=p)                    # node 8 keeps one child
    r = base["rows"].copy(); r[2, 2] = 4; variant(rows=r)                     # a row value of dim
    r = base["rows"].copy(); r[2, 2] = -3; variant(rows=r)
    return bad


def test_host_loop_equals_the_statement(tmp_path):
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_test.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    cases = [R.make_case(*k) for k in NATIVE_CASES]
    bad = _bad_cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % (len(cases) + len(bad)))
        for c in cases:
            f.write(_case_text(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["P"], c["derivs"]))
        for c in bad:
            f.write(_case_text(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["P"], c["derivs"]))
    # (-fno-sanitize=vptr: the unit holds Backend::tree_likelihood, and the check wants Backend's type information, which lives with
    #  the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(tmp_path / ("treelik_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}   # (both compilers at once)
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    for name in flags:
        exe = str(tmp_path / ("treelik_test_" + name))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % (len(cases) + len(bad))), r.stdout[-500:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        for k, c in enumerate(cases):
            l, kk, d1, d2 = (lines[4 * k + q].split() for q in range(4))
            want = c["want"]
            assert R.same_bits(np.array([float.fromhex(x) for x in l]), want["site_l"]), (name, NATIVE_CASES[k])
            assert np.array_equal(np.array([int(x) for x in kk], np.int32), want["site_k"]), (name, NATIVE_CASES[k])
            got1, got2 = (np.array([float.fromhex(x) for x in d]) for d in (d1, d2))
            if c["derivs"]:
                assert R.same_bits(got1, want["d1"]) and R.same_bits(got2, want["d2"]), (name, NATIVE_CASES[k])
            else:
                assert np.all(got1 == -7.5) and np.all(got2 == -7.5)   # untouched
        assert all(line.startswith("rejected tree likelihood:") for line in lines[4 * len(cases):-1]) and len(lines) == 4 * len(cases) + len(bad) + 1


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def run_ml(exe, fa, d, tag, opts=(), sites=True, env=None, ml=True):
    p = {k: os.path.join(str(d), "%s.%s" % (tag, k)) for k in ("tree", "sites")}
    args = ["--fasta", "--stats"] + (["--ml_tree", p["tree"]] if ml else []) + (["--ml_sites", p["sites"]] if ml and sites else [])
    r = bu.run(exe, args + list(opts) + [fa], env)
    read = lambda k: open(p[k]).read() if os.path.exists(p[k]) else None
    return SimpleNamespace(stdout=r.stdout, stats=bu.stats_of(r.stderr), stderr=r.stderr, **{k: read(k) for k in p})


def parse_fasta(text):
    seqs, name = {}, None
    for line in text.splitlines():
        if line.startswith(">"):
            name = line[1:].strip(); seqs[name] = ""
        elif name is not None:
            seqs[name] += line.strip()
    return seqs


def check_files(run, kind, model):
    """`--ml_sites` and ml_lnl against treelik_ref on the written tree and the written FASTA.
    formatNewick() prints 6 significant digits, coarser than 1e-9: a written length t differs from the optimiser's by at most
    5e-6 t, so a column's value may differ by sum_e |g_e| 5e-6 t_e to first order; the bound takes twice that (the second-order
    term, sum_e (|h_e| + g_e^2) (5e-6 t_e)^2 times the number of edges, is orders below) plus the 1e-9 relative of the statement.
    g, h: treelik_ref's own per-site ratios.  Returns (the reference's result, names, parent, lengths)."""
    Q, pi = model
    names, parent, lengths = R.from_newick(run.tree)
    rows = R.rows_of(parse_fasta(run.stdout), names, kind)
    want = R.evaluate(len(pi), len(names), parent, rows, pi, R.matrices(Q, lengths))
    ref = R.site_lnl(want["site_l"], want["site_k"])
    delta = 5e-6 * lengths
    bound = 2 * (np.abs(want["g"]) * delta[:, None]).sum(axis=0) + 1e-9 * np.abs(ref) + 1e-12
    lines = run.sites.splitlines()
    assert lines[0].startswith("lnL ") and len(lines) == 1 + rows.shape[1]
    got = []
    for c, line in enumerate(lines[1:]):
        col, value = line.split("\t")
        assert int(col) == c + 1
        got.append(float(value))
    got = np.array(got)
    worst = float(np.max(np.abs(got - ref) / bound))
    print("largest column difference over its bound: %.3g" % worst)
    assert worst <= 1.0
    total = float(lines[0].split()[1])
    assert lines[0] == "lnL %.17g" % run.stats["ml_lnl"]
    assert abs(total - float(np.sum(ref))) <= float(np.sum(bound))
    assert abs(total - float(np.sum(got))) <= 1e-9 * abs(total)
    return want, names, parent, lengths


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("ml_fams")
    all_fams = bu.aa_families(d)
    fams = {n: [f for f in all_fams if f.endswith("_n%d.fa" % n)][0] for n in (2, 3, 5, 8, 13, 24)}
    fams["5m"] = [f for f in all_fams if f.endswith("_n5.fa")][0]   # (the family whose rows carry a start character)
    fams["8x200"] = os.path.join(str(d), "fam_8x200.fa")
    with open(fams["8x200"], "w") as f:
        f.write(gen.fasta([("A" + s[1:]) if s[0] == "M" else s for s in gen.gen(8, 200, 77)]))
    fams["dna"] = bu.dna_families(d)
    fams["codon"] = bu.codon_families(d)
    fams["hky"] = bu.hky_model(d)
    return fams


@pytest.fixture(scope="module")
def wag():
    return R.shipped("wag.qmat")


def test_refusals(exe, fams, tmp_path):
    fa = fams[5]
    tree, sites = str(tmp_path / "never.tree"), str(tmp_path / "never.sites")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    topo = str(tmp_path / "topo.nwk")
    with open(topo, "w") as f:
        f.write(bu.run(exe, ["-T", "-i", "0", fa]).stdout)
    ml = ["--ml_tree", tree]
    cases = [
        (["--ml_sites", sites, fa], "need --ml_tree"),
        (["--ml_rounds", "5", fa], "need --ml_tree"),
        (["--ml_epsilon", "0.1", fa], "need --ml_tree"),
        (ml + [fams[2]], "at least 3 sequences"),
        (ml + ["--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_sites", sites, "--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_rounds", "5", "--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_epsilon", "0.1", "--batch", lst], "--batch cannot be combined with --ml_tree"),
        (ml + ["-W", fa], "cannot be combined with -W"),
        (ml + ["-r", fa], "cannot be combined with -r"),
        (ml + ["-rr", fa], "cannot be combined with -r"),
        (ml + ["--topology", topo, fa], "cannot be combined with --topology"),
    ]
    for bad in ("0", "-1", "10001", "abc", "", "1.5", "3x", "1e2"):
        cases.append((ml + ["--ml_rounds", bad, fa], "from 1 to 10000"))
    for bad in ("-0.1", "-1", "nan", "NaN", "-nan", "inf", "-inf", "abc", "", "0.3x"):
        cases.append((ml + ["--ml_epsilon", bad, fa], "X >= 0"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [p for p in os.listdir(str(tmp_path)) if p.startswith("never") or p == "b.out"]
        assert left == [], (args, left)


def test_other_outputs_unchanged_and_stats(exe, fams, tmp_path):
    for n in (5, 13):
        plain = bu.run(exe, ["--fasta", "--stats", fams[n]])
        r = run_ml(exe, fams[n], tmp_path, "ml%d" % n)
        assert r.stdout == plain.stdout and len(r.stdout) > 0
        assert not any(k in bu.stats_of(plain.stderr) for k in KEYS) and all(k in r.stats for k in KEYS)
        assert r.stats["ml_kernel_ms"] == 0 and r.stats["ml_tree_s"] > 0 and r.stats["ml_evaluations"] > r.stats["ml_rounds"] >= 1
        assert r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]
        bs = lambda tag, extra: (bu.run(exe, ["--fasta", "--bootstrap", "4", "--bootstrap_out", str(tmp_path / tag)] + extra + [fams[n]]).stdout, open(str(tmp_path / tag)).read())
        assert bs("b0", []) == bs("b1", ["--ml_tree", str(tmp_path / "b1.tree"), "--ml_sites", str(tmp_path / "b1.sites")])
        assert open(str(tmp_path / "b1.tree")).read() == r.tree and open(str(tmp_path / "b1.sites")).read() == r.sites   # independent of --bootstrap
        alone = run_ml(exe, fams[n], tmp_path, "alone%d" % n, sites=False)
        assert alone.tree == r.tree and alone.sites is None
        explicit = run_ml(exe, fams[n], tmp_path, "explicit%d" % n, ["--ml_rounds", "100", "--ml_epsilon", "1e-4"])   # the defaults
        assert (explicit.tree, explicit.sites) == (r.tree, r.sites)
        # -T prints what it prints without the flags; the tree is the one of the final alignment computed for the flag alone
        t = run_ml(exe, fams[n], tmp_path, "t%d" % n, ["-T", "-i", "0"])
        assert t.stdout == bu.run(exe, ["-T", "-i", "0", fams[n]]).stdout
        assert t.tree == run_ml(exe, fams[n], tmp_path, "u%d" % n, ["-i", "0"]).tree
        for switch in ("PGM_HOST_TREELIK", "PGM_DEVICE_TREELIK"):   # (this driver's backend has the default body: the host loop either way)
            h = run_ml(exe, fams[n], tmp_path, switch, env=dict(os.environ, **{switch: "1"}))
            assert (h.tree, h.sites) == (r.tree, r.sites) and switch in h.stats["switches"]


@pytest.mark.parametrize("n", [3, 5, "5m", 8, 24])
def test_topology_and_files(exe, fams, tmp_path, wag, n):
    r = run_ml(exe, fams[n], tmp_path, "f", ["-i", "0"])
    start = bu.run(exe, ["-T", "-i", "1", fams[n]]).stdout
    assert R.shape_of(r.tree) == R.shape_of(start) and r.tree.count(",") == start.count(",")
    assert r.tree != start and r.tree.endswith(";\n") and r.tree.count("\n") == 1
    _, _, _, lengths = check_files(r, "aa", wag)
    assert np.all(lengths >= 0.99e-6) and np.all(lengths <= 10.0)
    assert r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]


def test_likelihood_rises_from_a_p_distance_tree(exe, fams, tmp_path, wag):
    """8 sequences x 200 columns, the start tree from p-distances (no -m): strictly above the start, and the start is the
    likelihood of the BioNJ tree `-T` prints (within what its 6 digits allow: here 1e-4 relative)."""
    r = run_ml(exe, fams["8x200"], tmp_path, "p", ["-i", "0"])
    assert r.stats["ml_lnl"] > r.stats["ml_lnl_start"]
    check_files(r, "aa", wag)
    names, parent, lengths = R.from_newick(bu.run(exe, ["-T", "-i", "1", fams["8x200"]]).stdout)
    rows = R.rows_of(parse_fasta(r.stdout), names, "aa")
    want = R.evaluate(20, 8, parent, rows, wag[1], R.matrices(wag[0], np.clip(lengths, R.T_MIN, R.T_MAX), False), derivs=False)
    assert abs(R.lnl_of(want["site_l"], want["site_k"]) - r.stats["ml_lnl_start"]) < 1e-4 * abs(r.stats["ml_lnl_start"])
    one = run_ml(exe, fams["8x200"], tmp_path, "one", ["-i", "0", "--ml_rounds", "1"])
    assert one.stats["ml_rounds"] == 1 and 2 <= one.stats["ml_evaluations"] <= 12
    assert r.stats["ml_lnl"] > one.stats["ml_lnl"] > one.stats["ml_lnl_start"] == r.stats["ml_lnl_start"]
    check_files(one, "aa", wag)
    loose = run_ml(exe, fams["8x200"], tmp_path, "loose", ["-i", "0", "--ml_epsilon", "1000"])   # the first accepted gain is below it
    assert loose.stats["ml_rounds"] == 1 and loose.tree == one.tree


def test_dna_custom_model_and_codon(exe, fams, tmp_path):
    hky = R.custom(fams["hky"], 4)
    assert np.max(np.abs(hky[1] @ hky[0])) > 1e-3   # pi Q != 0: the generator is not reversible with respect to the frequencies used
    for k, fa in enumerate(fams["dna"]):
        if len(R.read_fasta(fa)) < 3:
            continue
        r = run_ml(exe, fa, tmp_path, "dna%d" % k, ["--dna", "--custom_model", fams["hky"]])
        check_files(r, "dna", hky)
        assert r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]
    ecm = R.shipped("ecm.qmat")
    for k, fa in enumerate(fams["codon"][:2]):
        r = run_ml(exe, fa, tmp_path, "cod%d" % k, ["--codon", "--ml_rounds", "3"])
        check_files(r, "codon", ecm)
        assert r.stats["ml_lnl"] >= r.stats["ml_lnl_start"]


@pytest.mark.parametrize("n", [5, 8])
def test_optimum_against_scipy(exe, fams, tmp_path, wag, n):
    """--ml_epsilon 0 --ml_rounds 2000 against scipy.optimize.minimize (L-BFGS-B, the same bounds, the same start) on treelik_ref's
    lnL.  The noise floor is the largest central-difference gradient entry of treelik_ref at scipy's optimum (edges not at a bound,
    the two root edges as one parameter).  The driver's lnL may be below scipy's by what that floor allows over the distance between
    the two optima, and its own largest gradient entry must be within 100 x the floor (the two stop by different rules)."""
    from scipy.optimize import minimize
    fa = fams[n] if n != 8 else fams["8x200"]
    Q, pi = wag
    r = run_ml(exe, fa, tmp_path, "opt", ["-i", "0", "--ml_epsilon", "0", "--ml_rounds", "2000"])
    assert r.stats["ml_rounds"] < 2000
    names, parent, ours = R.from_newick(r.tree)
    _, parent0, start = R.from_newick(bu.run(exe, ["-T", "-i", "1", fa]).stdout)
    assert np.array_equal(parent, parent0)
    rows = R.rows_of(parse_fasta(r.stdout), names, "aa")
    nleaves = len(names)

    def lnl(t, derivs=False):
        res = R.evaluate(20, nleaves, parent, rows, pi, R.matrices(Q, t, derivs), derivs)
        return (R.lnl_of(res["site_l"], res["site_k"]), res.get("d1"))

    def objective(t):
        value, d1 = lnl(t, True)
        return -value, -d1

    start = np.clip(start, R.T_MIN, R.T_MAX)
    sp = minimize(objective, start, jac=True, method="L-BFGS-B", bounds=[(R.T_MIN, R.T_MAX)] * len(start))
    root_edges = [e for e in range(len(parent) - 1) if int(parent[e]) == len(parent) - 1]

    def entries(t, grad):
        """|gradient| per free parameter: the edges not at a bound; the root edges (a bifurcating root) as one."""
        free = lambda e: R.T_MIN * 1.01 < t[e] < R.T_MAX * 0.99
        out = [abs(grad[e]) for e in range(len(t)) if e not in root_edges and free(e)]
        if len(root_edges) == 2:
            g = [grad[e] for e in root_edges if free(e)]
            out += [abs(sum(g) / len(g))] if g else []
        else:
            out += [abs(grad[e]) for e in root_edges if free(e)]
        return max(out) if out else 0.0

    step = 1e-4
    cd = np.zeros(len(start))
    for e in range(len(start)):
        up, dn = sp.x.copy(), sp.x.copy()
        up[e] = min(R.T_MAX, up[e] + step); dn[e] = max(R.T_MIN, dn[e] - step)
        cd[e] = (lnl(up)[0] - lnl(dn)[0]) / (up[e] - dn[e])
    floor = entries(sp.x, cd)
    ours_lnl, ours_d1 = lnl(ours, True)
    mine = entries(ours, ours_d1)
    allowed = floor * float(np.abs(ours - sp.x).sum()) + 1e-9 * abs(sp.fun)
    print("taxa %d: lnL driver %.12g (statement on the written tree %.12g), scipy %.12g; noise floor %.3g, driver's largest gradient entry %.3g, allowed deficit %.3g"
          % (n, r.stats["ml_lnl"], ours_lnl, -sp.fun, floor, mine, allowed))
    assert floor > 0
    assert r.stats["ml_lnl"] >= -sp.fun - allowed
    assert mine <= 100 * floor
