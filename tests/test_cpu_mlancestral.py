"""`--ml_ancestral`, `--ml_ancestral_tree` and `--ml_ancestral_probs` through the CPU oracle driver (pgmsa_oracle: Backend::tree_ancestral's
default, the host loop), and the pieces below it:
  - tests/treelik_anc_ref.py itself against brute force (every assignment of the inner nodes' states enumerated), and its properties;
  - tree_ancestral_host in a stand-alone program (tests/native/treelik_anc_test.cpp), its %a output equal to the statement bit for
    bit; built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, every other output unchanged, the stats key, the three files against the statement on the written tree and
    the written FASTA, the gap rule, the alphabets."""
import itertools
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import gen
import mldist_general_ref as M
import test_cpu_mlgamma as TG
import test_cpu_mltree as TM
import test_cpu_treelik_shapes as SH
import transfer_ref as T
import treelik_anc_ref as A
import treelik_rates_ref as G
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52


# ---- the statement against brute force ---------------------------------------------------------------------------------------------------
def brute(dim, nleaves, parent, rows, pi, w, mats):
    """mats[c][e][i, j]: parent state i -> child state j.  The joint of every assignment of the inner nodes' states, summed: returns
    (site_l, anc) with anc[v - nleaves][s, i] = sum_c w_c Pr(x_v = i, data | c) / sum_c w_c Pr(data | c)."""
    nnodes, ncols = len(parent), rows.shape[1]
    ninner, root = nnodes - nleaves, nnodes - 1
    site_l, num = np.zeros(ncols), np.zeros((ninner, ncols, dim))
    for s in range(ncols):
        for c in range(len(w)):
            for x in itertools.product(range(dim), repeat=ninner):
                p = pi[x[root - nleaves]]
                for v in range(root):
                    row = mats[c][v][x[int(parent[v]) - nleaves]]
                    if v >= nleaves:
                        p = p * row[x[v - nleaves]]
                    else:
                        p = p * (row.sum() if rows[v, s] < 0 else row[rows[v, s]])
                site_l[s] += w[c] * p
                for v in range(ninner):
                    num[v, s, x[v]] += w[c] * p
    return site_l, num / site_l[None, :, None]


BRUTE = [(4, "two", 1), (4, "two", 2), (4, "three", 1), (4, "three", 2), (4, "tri", 1), (4, "tri", 2), (4, "five", 1), (4, "five", 2), (20, "three", 1), (20, "three", 2)]


@pytest.mark.parametrize("dim,tree,ncat", BRUTE)
def test_reference_against_brute_force(dim, tree, ncat):
    """site_l and every posterior within 1e-10 relative of the enumeration (the tolerance tests/test_cpu_mlgamma.py takes for the site
    likelihoods; measured here: below 3e-15 for both), scipy's expm per category and edge, columns with gaps and -2 among them."""
    from scipy.linalg import expm
    rng = np.random.default_rng(100 * dim + ncat + sum(map(ord, tree)))
    nleaves, parent = {"two": (2, R.balanced(2)), "three": (3, R.caterpillar(3)), "tri": (5, R.trifurcating(5)), "five": (5, R.balanced(5))}[tree]
    nedges = len(parent) - 1
    if tree == "tri":
        assert sum(int(p) == len(parent) - 1 for p in parent) == 3
    Q = M.random_generator(dim, 40 + dim)   # (not reversible)
    pi = rng.dirichlet(np.ones(dim) * 3)
    lengths = rng.uniform(0.05, 0.6, nedges)
    ncols = 6 if dim == 4 else 4
    rows = rng.integers(0, dim, (nleaves, ncols)).astype(np.int8)
    rows[0, 1] = -1; rows[:, 2] = -1; rows[nleaves - 1, 3] = -2
    rates, w = (np.array([1.0]), np.array([1.0])) if ncat == 1 else (np.array([0.3, 1.9]), np.array([0.35, 0.65]))
    got = A.evaluate(dim, nleaves, parent, rows, pi, w, G.matrices(Q, lengths, rates, derivs=False))
    want_l, want = brute(dim, nleaves, parent, rows, pi, w, [[expm(Q * r * t) for t in lengths] for r in rates])
    assert np.all(got["site_k"] == 0) and np.all(want > 0)
    dl, da = float(np.max(np.abs(got["site_l"] - want_l) / want_l)), float(np.max(np.abs(got["anc_post"] - want) / want))
    print("largest relative difference: site_l %.3g, posteriors %.3g" % (dl, da))
    assert dl < 1e-10 and da < 1e-10
    assert np.array_equal(got["anc_state"], np.argmax(want, axis=2)) and np.max(np.abs(got["anc_prob"] - want.max(axis=2))) < 1e-10


# ---- properties of the statement -----------------------------------------------------------------------------------------------------------
PROPERTY_CASES = [(4, 33, "balanced8", 1), (4, 33, "balanced8", 4), (20, 17, "balanced8", 2), (61, 15, "trifurcating", 4), (64, 17, "balanced8", 16), (20, 33, "balanced24", 4),
                  (4, 33, "three", 4), (4, 33, "two", 4)]


@pytest.mark.parametrize("key", PROPERTY_CASES)
def test_posteriors_sum_to_one(key):
    """Every category's vector and every mixed vector sums to 1 within dim ulps of 1 (the sums here in extended precision)."""
    want = A.make_case(*key)["want"]
    dim = key[0]
    for name in ("cat_a", "anc_post"):
        total = want[name].astype(np.longdouble).sum(axis=-1)
        worst = float(np.max(np.abs(total - 1)))
        print("%s: largest |sum - 1| = %.3g ulps" % (name, worst / ULP))
        assert worst <= dim * ULP, name
    assert np.all(want["anc_state"] >= 0) and np.all(want["anc_prob"] > 0)


@pytest.mark.parametrize("key", PROPERTY_CASES)
def test_site_values_are_those_without_derivatives(key):
    want, old = A.make_case(*key)["want"], G.make_case(*key, False)["want"]
    for k in ("site_l", "site_k", "post"):
        assert R.same_bits(want[k], old[k]), k
    assert np.array_equal(want["anc_state"], np.argmax(want["anc_post"], axis=2))   # (numpy's argmax: the first index of the maximum)
    assert R.same_bits(want["anc_prob"], want["anc_post"].max(axis=2))


@pytest.mark.parametrize("dim", [4, 20, 61])
def test_column_of_gaps_gives_the_frequencies(dim):
    """Under a generator whose stationary distribution is pi (here Q = S diag(pi), S symmetric and seeded; the shipped models keep the
    reference's frequencies, which are not stationary under their Q, so there only the root has pi) a column of gaps has pi at every
    node, up to what the matrices miss: e = the largest of |row sum - 1| and |(pi P - pi) / pi| over the edges, measured here on the
    matrices themselves.  Asserted: |a - pi| / pi and |site_l - 1| within 10 * e.  Measured: e up to 3.0e-15, the largest |a - pi| / pi
    up to 2.4e-15 (0.4 to 1.8 times e)."""
    rng = np.random.default_rng(30 + dim)
    pi = rng.dirichlet(np.ones(dim) * 4)
    S = rng.uniform(0.1, 2.0, (dim, dim))
    Q = (S + S.T) * pi[None, :]
    Q = M.normalised(Q, pi)
    nleaves, parent = R.TREES["balanced8"]()
    nedges = len(parent) - 1
    lengths = rng.uniform(0.02, 1.5, nedges)
    rows = rng.integers(0, dim, (nleaves, 3)).astype(np.int8)
    rows[:, 1] = -1
    for rates, w in ((np.array([1.0]), np.array([1.0])), (np.array([0.2, 0.7, 1.1, 2.0]), np.full(4, 0.25))):
        P = G.matrices(Q, lengths, rates, derivs=False)
        X = np.asarray(P).reshape(len(w), nedges, dim, dim).transpose(0, 1, 3, 2)
        e = max(float(np.max(np.abs(X.sum(axis=3) - 1))), float(np.max(np.abs((pi[None, None, :, None] * X).sum(axis=2) - pi) / pi)))
        got = A.evaluate(dim, nleaves, parent, rows, pi, w, P)
        diff = float(np.max(np.abs(got["anc_post"][:, 1, :] - pi) / pi))
        print("dim %d, %d categories: e = %.3g, largest |a - pi| / pi = %.3g" % (dim, len(w), e, diff))
        assert e < 1e-13 and diff <= 10 * e
        assert abs(got["site_l"][1] - 1) <= 10 * e
        assert np.max(np.abs(got["anc_post"][:, 0, :] - pi)) > 1e-3   # (a column with residues is another matter)


@pytest.mark.parametrize("key", [(4, 33, "balanced8"), (20, 17, "trifurcating"), (61, 15, "balanced8")])
def test_one_category_root_is_pi_times_partial(key):
    """ncat == 1: the root's vector is pi(i) U_root(i) / site_l; U_root here by plain matrix products (within 1e-12 relative)."""
    c = A.make_case(*key, 1)
    dim, nleaves, parent, rows = c["dim"], c["nleaves"], c["parent"], c["rows"]
    X = R.unpack(c["P"], len(parent) - 1, 1, dim)
    kids = R.children_of(parent)
    U = [((rows[l][:, None] < 0) | (rows[l][:, None] == np.arange(dim)[None, :])).astype(np.float64) for l in range(nleaves)]
    for v in range(nleaves, len(parent)):
        U.append(np.prod([U[k] @ X[k][0].T for k in kids[v]], axis=0))
    want = c["pi"][None, :] * U[-1] / c["want"]["site_l"][:, None]
    assert np.all(c["want"]["site_k"] == 0) and np.all(c["want"]["post"] == 1.0)
    assert np.max(np.abs(c["want"]["anc_post"][-1] - want) / want) < 1e-12
    assert R.same_bits(c["want"]["anc_post"], c["want"]["cat_a"][0])   # (1.0 * x and 0.0 + x are exact)


def tie_case():
    """Two leaves under the root, every matrix entry 0.25 (row sums exactly 1), pi = (1/8, 3/8, 3/8, 1/8): the root's vector is pi
    exactly whatever the leaves hold, states 1 and 2 tie, and the first wins."""
    return dict(dim=4, nleaves=2, parent=np.array([2, 2, R.ROOT], np.uint32), rows=np.array([[0, -1, 3, -2], [1, -1, 3, 2]], np.int8), pi=np.array([0.125, 0.375, 0.375, 0.125]),
                w=np.array([0.5, 0.5]), P=np.full(2 * 2 * 16, 0.25), tree="tie", ncat=2)


def zero_case():
    """Category 0 has identity matrices and the two leaves differ in columns 0 and 2, so every partial and every Z of it is 0.0 there
    (no NaN among the inputs or the outputs): its posterior share is 0.0 and the mixture is category 1's vector.  Columns 1 and 3
    are possible under both categories."""
    rng = np.random.default_rng(8)
    P1 = rng.uniform(0.01, 1.0, (2, 4, 4))
    P1 /= P1.sum(axis=2, keepdims=True)
    P = np.concatenate([R.pack(np.stack([np.eye(4), np.eye(4)])[:, None]), R.pack(P1[:, None])])
    return dict(dim=4, nleaves=2, parent=np.array([2, 2, R.ROOT], np.uint32), rows=np.array([[0, 2, 1, -1], [1, 2, 3, 0]], np.int8), pi=np.array([0.1, 0.2, 0.3, 0.4]),
                w=np.array([0.5, 0.5]), P=P, tree="zero", ncat=2)


def with_want(c):
    c = dict(c)
    c["want"] = A.evaluate(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"])
    return c


def test_ties_go_to_the_first_index():
    want = with_want(tie_case())["want"]
    assert np.all(want["anc_post"][0] == np.array([0.125, 0.375, 0.375, 0.125])[None, :])
    assert np.all(want["anc_state"] == 1) and np.all(want["anc_prob"] == 0.375)


def test_zero_rule():
    """Z == 0.0: a category whose likelihood of the column is 0.0 contributes 0.0, not 0.0 * NaN."""
    c = with_want(zero_case())
    want = c["want"]
    assert not np.any(np.isnan(want["anc_post"])) and not np.any(np.isnan(want["post"]))
    hit = np.array([True, False, True, False])
    assert np.all(want["cat_a"][0][:, hit, :] == 0.0) and np.all(want["post"][0][hit] == 0.0) and np.all(want["post"][1][hit] == 1.0)
    assert R.same_bits(want["anc_post"][:, hit, :], want["cat_a"][1][:, hit, :])
    assert np.all(want["cat_a"][0][0, 1] == np.array([0.0, 0.0, 1.0, 0.0]))
    one = with_want(dict(c, w=np.array([1.0]), P=c["P"][:32], ncat=1))["want"]   # category 0 alone: site_l == 0.0, post NaN, no state
    assert np.all(one["site_l"][hit] == 0.0) and np.all(one["anc_state"][0, hit] == -1) and np.all(one["anc_prob"][0, hit] == 0.0)
    assert np.all(one["anc_state"][0, ~hit] >= 0)


def presence_case():
    """((0,1)5,((2,3)6,4)7)8.  x: a residue, -: a gap (a row of -2 counts as a residue).  Returns a case (seeded matrices: the rule
    does not read them) and the expected pattern, written out by hand."""
    parent = np.array([5, 5, 6, 6, 7, 8, 7, 8, R.ROOT], np.uint32)
    text = ["xx---x-",    # leaf 0
            "x-x--x-",    # leaf 1
            "x-xx---",    # leaf 2
            "x--x--x",    # leaf 3
            "x---x-x"]    # leaf 4
    rows = np.array([[0 if ch == "x" else -1 for ch in line] for line in text], np.int8)
    rows[0, 0] = -2
    # the pattern, written out per column (rows: nodes 5, 6, 7, 8):
    #  col 0: everyone has a residue -> every node
    #  col 1: leaf 0 alone -> no node
    #  col 2: leaves 1 and 2 -> the path 1 - 5 - 8 - 7 - 6 - 2: nodes 5, 8, 7, 6
    #  col 3: leaves 2 and 3 -> node 6 alone
    #  col 4: leaf 4 alone -> no node
    #  col 5: leaves 0 and 1 -> node 5 alone
    #  col 6: leaves 3 and 4 -> the path 3 - 6 - 7 - 4: nodes 6, 7
    want = np.array([[1, 0, 1, 0, 0, 1, 0],
                     [1, 0, 1, 1, 0, 0, 1],
                     [1, 0, 1, 0, 0, 0, 1],
                     [1, 0, 1, 0, 0, 0, 0]], bool)
    rng = np.random.default_rng(21)
    P0 = rng.uniform(0.01, 1.0, (8, 4, 4))
    P0 /= P0.sum(axis=2, keepdims=True)
    return dict(dim=4, nleaves=5, parent=parent, rows=rows, pi=np.array([0.1, 0.2, 0.3, 0.4]), w=np.array([1.0]), P=R.pack(P0[:, None]), tree="hand-made", ncat=1), want


def test_presence_rule_on_a_hand_made_alignment():
    """The statement's rule on the hand-written pattern; test_host_loop_equals_the_statement puts the same pattern to the C++ rule."""
    case, want = presence_case()
    assert np.array_equal(A.presence(5, case["parent"], case["rows"]), want)


# ---- the host loop, stand-alone ----------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_mlancestral.py, which takes these lists from here: the host loop runs every one of them.
DIMS = (4, 20, 61, 64)
GRID = [(dim, ncols, "balanced8", ncat) for dim in DIMS for ncat in (1, 2, 4, 16) for ncols in (1, 17, 33)]
OTHER_TREES = [(dim, 33, tree, 4) for dim in DIMS for tree in ("two", "three", "balanced24", "trifurcating")]
MANY_COLUMNS = (4, 300, "balanced8", 4)
MIXED_SCALING = [(4,), (4, 1e-6, 5), (20, 1e-6, 5)]
UNEQUAL = (4, 33, "balanced8", 4, "unequal")
NOT_FULL = [(20, 33, "balanced8", 4), (61, 17, "balanced8", 2), (4, 17, "balanced24", 16), (64, 33, "trifurcating", 4)]   # without anc_post
ONE_CATEGORY = [(4, 33, "balanced8", 1), (20, 17, "balanced8", 1), (61, 33, "trifurcating", 1), (64, 17, "balanced24", 1)]
MIXED_SHAPES = [(20, 33, "balanced8", 16), (4, 1, "balanced8", 2), (64, 33, "balanced24", 4), (4, 300, "balanced8", 4), (4, 17, "balanced8", 1)]
SMALL_VALID = (4, 15, "balanced8", 2)   # what the rejections change
NATIVE_CASES = list(dict.fromkeys(GRID + OTHER_TREES + [MANY_COLUMNS] + ONE_CATEGORY + MIXED_SHAPES + NOT_FULL + [SMALL_VALID] + SH.NATIVE_ANC))   # (SH: the other dims, polytomies)


def _case_bytes(c, full=1, **kw):
    """One case of tests/native/treelik_anc_test.cpp's binary file (as text the dim-61 and dim-64 cases with 16 categories, 0.9
    million matrix entries each, would make a file of some 200 MB)."""
    d = dict(c); d.update(kw)
    nnodes = d.get("nnodes", len(d["parent"]))
    head = np.array([d["dim"], d["nleaves"], nnodes, d["rows"].shape[1], d["ncat"], full], np.int32)
    parts = [head, np.asarray(d["parent"], np.uint32), np.asarray(d["rows"], np.int8), np.asarray(d["pi"], np.float64), np.asarray(d["w"], np.float64), np.asarray(d["P"], np.float64)]
    return b"".join(np.ascontiguousarray(x).tobytes() for x in parts)


def _bad_cases():
    """What tree_ancestral_host refuses, each a change to one small valid case."""
    c = A.make_case(4, 15, "balanced8", 2)
    bad = []
    for ncat in (0, 17):
        bad.append(_case_bytes(c, ncat=ncat, w=np.full(ncat, 0.5), P=np.tile(c["P"][:len(c["P"]) // 2], ncat)))
    for v in (0.0, -0.5, float("nan"), float("inf")):
        bad.append(_case_bytes(c, w=np.array([0.5, v])))
    for b in TM._bad_cases():
        bad.append(_case_bytes(c, parent=b["parent"], rows=b["rows"]))
    return bad


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("anc_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_anc_test.cpp")] + [os.path.join(host, f) for f in TREELIK_HOST_SOURCES]
    hand, pattern = presence_case()
    cases = [A.make_case(*k) for k in NATIVE_CASES] + [A.make_case(*UNEQUAL)] + [A.make_mixed_scaling_case(*k) for k in MIXED_SCALING] + \
        [with_want(tie_case()), with_want(zero_case()), with_want(hand)]
    partial = [A.make_case(*k) for k in NOT_FULL]   # without anc_post
    bad = _bad_cases()
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases) + len(partial) + len(bad)], np.int32).tobytes())
        for c in cases:
            f.write(_case_bytes(c))
        for c in partial:
            f.write(_case_bytes(c, full=0))
        for blob in bad:
            f.write(blob)
    # (-fno-sanitize=vptr: as tests/test_cpu_mltree.py, the unit holds Backend's virtual defaults without the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("anc_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    for name in flags:
        r = subprocess.run([str(d / ("anc_test_" + name)), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % (len(cases) + len(partial) + len(bad))), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    return SimpleNamespace(cases=cases, partial=partial, bad=bad, lines=out, pattern=pattern)


def _compare(lines, case, what, full=True):
    floats = lambda text: np.array([float.fromhex(x) for x in text.split()])
    ints = lambda text, t: np.array([int(x) for x in text.split()], t)
    l, kk, post, state, prob, anc, present = lines
    want = case["want"]
    held = np.array([ch == "1" for ch in present]).reshape(want["anc_state"].shape)
    assert set(present) <= {"0", "1"} and np.array_equal(held, A.presence(case["nleaves"], case["parent"], case["rows"])), what   # the C++ gap rule
    assert R.same_bits(floats(l), want["site_l"]), what
    assert np.array_equal(ints(kk, np.int32), want["site_k"]), what
    assert R.same_bits(floats(post).reshape(want["post"].shape), want["post"]), what
    assert np.array_equal(ints(state, np.int8).reshape(want["anc_state"].shape), want["anc_state"]), what
    assert R.same_bits(floats(prob).reshape(want["anc_prob"].shape), want["anc_prob"]), what
    if full:
        assert R.same_bits(floats(anc).reshape(want["anc_post"].shape), want["anc_post"]), what
    else:
        assert np.all(floats(anc) == -7.5), what   # untouched


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_loop_equals_the_statement(native, build):
    lines, cases = native.lines[build], native.cases
    for k, c in enumerate(cases):
        _compare(lines[7 * k:7 * k + 7], c, (build, k, c["dim"], c["tree"], c["ncat"]))
    for k, c in enumerate(native.partial, len(cases)):
        _compare(lines[7 * k:7 * k + 7], c, (build, k, "without anc_post"), full=False)
    hand = lines[7 * (len(cases) - 1) + 6]   # the hand-made pattern, the last of `cases`
    assert np.array_equal(np.array([ch == "1" for ch in hand]).reshape(native.pattern.shape), native.pattern)
    first = 7 * (len(cases) + len(native.partial))
    rejected = lines[first:first + len(native.bad)]
    assert len(rejected) == len(native.bad) and all(line.startswith("rejected tree likelihood:") for line in rejected), rejected
    assert len(lines) == first + len(native.bad) + 1


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def run_a(exe, fa, d, tag, opts=(), tree=True, probs=True, env=None, anc=True):
    p = {k: os.path.join(str(d), "%s.%s" % (tag, k)) for k in ("anc", "anctree", "probs", "rates")}
    extra = (["--ml_ancestral", p["anc"]] if anc else []) + (["--ml_ancestral_tree", p["anctree"]] if tree else []) + (["--ml_ancestral_probs", p["probs"]] if probs else [])
    if "--ml_gamma" in opts:
        extra += ["--ml_rates", p["rates"]]
    r = TM.run_ml(exe, fa, d, tag, list(opts) + extra, env=env)
    for k in p:
        setattr(r, k, open(p[k]).read() if os.path.exists(p[k]) else None)
    return r


def labelled_newick(text):
    """--ml_ancestral_tree's line in ml_tree_topology's numbering: (names, parent, lengths per edge, label per inner node)."""
    text = text.strip()
    m = re.search(r"\)([^():,;]*);$", text)
    assert m, text[-40:]
    root = T.parse(text[:m.start(1)] + ";")
    names = sorted(T.leaves(root))
    index = {n: k for k, n in enumerate(names)}
    parent, length, label = [R.ROOT] * len(names), [None] * len(names), [None] * len(names)

    def walk(node, own):
        if isinstance(node, str):
            return index[node]
        ids = [(walk(kid, lab), float(ln[1:])) for kid, ln, lab in node]
        parent.append(R.ROOT); length.append(None); label.append(own)
        v = len(parent) - 1
        for c, t in ids:
            parent[c], length[c] = v, t
        return v

    walk(root, m.group(1))
    return names, np.array(parent, np.uint32), np.array(length[:-1], np.float64), label[len(names):]


def symbols_of(kind):
    if kind == "aa":
        return list(R._AA)
    if kind == "dna":
        return list("TCAG")
    out = []
    for c in range(64):
        if c not in (10, 11, 14):
            out.append("TCAG"[c // 16] + "TCAG"[(c // 4) % 4] + "TCAG"[c % 4])
    return out


def check_files(run, kind, model, K=0):
    """The three files against the statement on the written tree (--ml_ancestral_tree: the topology, the names and the lengths), the
    written alpha and the written FASTA.  Presence is integer work and must match exactly.  The newick's 6 digits move a length t by up
    to 5e-6 t; a posterior is a ratio of two sums of products of one entry of every edge's matrix, all positive, so it moves by at most
    (relative) 2 sum_e max_c eps_ce, eps_ce = the largest relative change of an entry of P(r_c t_e) = max |r_c (Q P)_ab / P_ab| 5e-6 t_e;
    the bound takes twice that (second order) plus 1e-9 (the matrices of the two sides: scipy's expm against the driver's).  A state
    must be the statement's where the statement's two largest posteriors are further apart than their bounds, and one of the states
    within the bounds of the largest elsewhere; its probability is compared under the same bound."""
    from scipy.linalg import expm
    Q, pi = model
    dim = len(pi)
    sym = symbols_of(kind)
    width = len(sym[0])
    names, parent, lengths, labels = labelled_newick(run.anctree)
    nleaves, ninner = len(names), len(parent) - len(names)
    assert labels == ["N%d" % (k + 1) for k in range(ninner)]
    plain = R.from_newick(run.tree)
    assert plain[0] == names and np.array_equal(plain[1], parent) and np.array_equal(plain[2], lengths)
    assert re.sub(r"\)N\d+", ")", run.anctree) == run.tree   # the --ml_tree line with the labels added
    rows = R.rows_of(TM.parse_fasta(run.stdout), names, kind)
    ncols = rows.shape[1]
    if K:
        alpha, rates, _ = TG.parse_rates(run.rates)
        rates, w = G.gamma_rates(alpha, K), G.weights_of(K)
    else:
        rates, w = np.array([1.0]), np.array([1.0])
    want = A.evaluate(dim, nleaves, parent, rows, pi, w, G.matrices(Q, lengths, rates, derivs=False))
    eps = np.zeros(len(lengths))
    for e, t in enumerate(lengths):
        for r in rates:
            Pm = expm(Q * r * t)
            eps[e] = max(eps[e], float(np.max(np.abs(r * (Q @ Pm) / Pm))) * 5e-6 * t)
    bound = 4 * float(eps.sum()) + 1e-9
    present = A.presence(nleaves, parent, rows)
    # the FASTA: one record per inner node in order, one line each
    recs = run.anc.splitlines()
    assert len(recs) == 2 * ninner and [recs[2 * k] for k in range(ninner)] == [">N%d" % (k + 1) for k in range(ninner)]
    lines = run.probs.splitlines()
    assert len(lines) == ninner * ncols
    compared, worst = 0, 0.0
    for k in range(ninner):
        seq = recs[2 * k + 1]
        assert len(seq) == width * ncols
        for s in range(ncols):
            name, col, text, prob, held = lines[k * ncols + s].split("\t")
            assert name == "N%d" % (k + 1) and int(col) == s + 1 and held == ("1" if present[k, s] else "0")
            assert text in sym
            assert seq[width * s:width * s + width] == (text if present[k, s] else "-" * width)
            state, p = sym.index(text), float(prob)
            post = want["anc_post"][k, s]
            top = float(post.max())
            assert "%.17g" % p == prob
            near = np.flatnonzero(post >= top * (1 - bound) / (1 + bound))
            assert state in near, (k, s, state, near)
            if len(near) == 1:
                compared += 1
            worst = max(worst, abs(p - post[state]) / post[state] / bound)
    print("%d of %d states compared exactly; largest probability difference over the bound (%.3g relative): %.3g" % (compared, ninner * ncols, bound, worst))
    assert worst <= 1.0 and compared >= 0.9 * ninner * ncols
    return want, names, parent, rows, present


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mla_fams")
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
    p = lambda k: str(tmp_path / ("never." + k))
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    ml = ["--ml_tree", p("tree")]
    anc = ["--ml_ancestral", p("anc")]
    cases = [
        (anc + [fa], "--ml_ancestral needs --ml_tree"),
        (anc + ["--ml_ancestral_tree", p("at"), "--ml_ancestral_probs", p("ap"), fa], "--ml_ancestral needs --ml_tree"),
        (["--ml_ancestral_tree", p("at"), fa], "--ml_ancestral needs --ml_tree"),
        (ml + ["--ml_ancestral_tree", p("at"), fa], "--ml_ancestral_tree and --ml_ancestral_probs need --ml_ancestral"),
        (ml + ["--ml_ancestral_probs", p("ap"), fa], "--ml_ancestral_tree and --ml_ancestral_probs need --ml_ancestral"),
        (ml + anc + ["--batch", lst], "--batch cannot be combined with --ml_tree"),
        (anc + ["--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_ancestral_probs", p("ap"), "--batch", lst], "--batch cannot be combined with --ml_tree"),
        # what the tests of the older flags pin stays as it is for its combination of flags, with the new ones beside them
        (anc + ["--ml_sites", p("sites"), fa], "--ml_sites, --ml_rounds and --ml_epsilon need --ml_tree"),
        (anc + ["--ml_gamma", "4", fa], "--ml_gamma, --ml_alpha and --ml_rates need --ml_tree"),
        (ml + anc + ["--ml_alpha", "0.5", fa], "--ml_alpha and --ml_rates need --ml_gamma"),
        (ml + anc + ["--ml_gamma", "1", fa], "from 2 to 16"),
        (ml + anc + ["-W", fa], "--ml_tree cannot be combined with -W"),
        (ml + anc + ["-r", fa], "--ml_tree cannot be combined with -r"),
        (ml + anc + [fams[2]], "at least 3 sequences"),
    ]
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [q for q in os.listdir(str(tmp_path)) if q.startswith("never") or q == "b.out"]
        assert left == [], (args, left)


def test_a_leaf_with_a_node_name_is_refused(exe, tmp_path):
    seqs = gen.gen(4, 60, 77)
    fa = str(tmp_path / "names.fa")
    with open(fa, "w") as f:
        for name, s in zip(["a", "N2", "b", "c"], seqs):
            f.write(">%s\n%s\n" % (name, s))
    r = subprocess.run([exe, "--fasta", "--ml_tree", str(tmp_path / "t"), "--ml_ancestral", str(tmp_path / "never.anc"), fa], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "N2" in r.stderr and "inner node" in r.stderr
    assert not os.path.exists(str(tmp_path / "never.anc")) and not os.path.exists(str(tmp_path / "t"))   # (before the optimiser and any file)
    ok = bu.run(exe, ["--fasta", "--ml_tree", str(tmp_path / "t"), fa])   # (without the flag the name is an ordinary one)
    assert ">N2" in ok.stdout


def test_other_outputs_unchanged_and_stats(exe, fams, tmp_path, wag):
    fa = fams[8]
    plain = bu.run(exe, ["--fasta", "--stats", fa])
    assert "ml_ancestral_s" not in bu.stats_of(plain.stderr)
    for tag, opts in (("p", []), ("g", ["--ml_gamma", "4"])):
        old = TG.run_g(exe, fa, tmp_path, "old" + tag, opts, rates=bool(opts))
        assert "ml_ancestral_s" not in old.stats
        new = run_a(exe, fa, tmp_path, "new" + tag, opts)
        assert new.stdout == plain.stdout == old.stdout and len(new.stdout) > 0
        assert (new.tree, new.sites, new.rates) == (old.tree, old.sites, old.rates) and len(new.tree) > 0
        assert new.stats["ml_ancestral_s"] > 0 and new.stats["ml_kernel_ms"] == 0
        assert sorted(set(new.stats) - set(old.stats)) == ["ml_ancestral_s"] and set(old.stats) <= set(new.stats)
        for k in ("ml_lnl", "ml_lnl_start", "ml_rounds", "ml_evaluations"):
            assert new.stats[k] == old.stats[k], k
        alone = run_a(exe, fa, tmp_path, "alone" + tag, opts, tree=False, probs=False)
        assert alone.anc == new.anc and alone.anctree is None and alone.probs is None
        for switch in ("PGM_HOST_TREELIK", "PGM_DEVICE_TREELIK"):   # (this driver's backend has the default body: the host loop either way)
            h = run_a(exe, fa, tmp_path, switch + tag, opts, env=dict(os.environ, **{switch: "1"}))
            assert (h.anc, h.anctree, h.probs) == (new.anc, new.anctree, new.probs)
    bs = lambda tag, extra: (bu.run(exe, ["--fasta", "--bootstrap", "4", "--bootstrap_out", str(tmp_path / tag)] + extra + [fa]).stdout, open(str(tmp_path / tag)).read())
    with_flags = bs("b1", ["--ml_tree", str(tmp_path / "b1.tree"), "--ml_ancestral", str(tmp_path / "b1.anc"), "--ml_ancestral_tree", str(tmp_path / "b1.at")])
    assert bs("b0", []) == with_flags   # (the labelled formatter leaves the bootstrap's text as it was)


@pytest.mark.parametrize("n,opts", [(5, []), (5, ["--ml_gamma", "4"]), (13, []), (8, ["--ml_gamma", "4", "--ml_alpha", "0.7"])])
def test_files_aa(exe, fams, tmp_path, wag, n, opts):
    """Amino acids with and without --ml_gamma; the family of 5 has a re-inserted start column (an X where M was stripped)."""
    r = run_a(exe, fams[n], tmp_path, "f", ["-i", "0"] + opts)
    want, names, parent, rows, present = check_files(r, "aa", wag, 4 if opts else 0)
    if n == 5:
        seqs = TM.parse_fasta(r.stdout)
        first = {name: seqs[name][0] for name in names}
        assert set(first.values()) == {"M", "-"}   # the start column as written
        held = [k for k, name in enumerate(names) if first[name] == "M"]
        assert len(held) >= 2 and np.array_equal(rows[:, 0] >= 0, np.array([first[name] == "M" for name in names]))
        assert present[:, 0].any()   # (which nodes: the rule on the written tree, compared in check_files)
    full = (rows != -1).all(axis=0)
    assert full.any() and present[:, full].all()
    lone = (rows != -1).sum(axis=0) == 1
    assert not present[:, lone].any()


def test_dna_custom_model_and_codon(exe, fams, tmp_path):
    hky = R.custom(fams["hky"], 4)
    fa = [f for f in fams["dna"] if len(R.read_fasta(f)) >= 3][0]
    r = run_a(exe, fa, tmp_path, "dna", ["--dna", "--custom_model", fams["hky"]])
    check_files(r, "dna", hky)
    ecm = R.shipped("ecm.qmat")
    r = run_a(exe, fams["codon"][1], tmp_path, "cod", ["--codon", "--ml_rounds", "3", "--ml_gamma", "2"])
    want, names, parent, rows, present = check_files(r, "codon", ecm, 2)
    assert all(len(line) == 3 * rows.shape[1] for line in r.anc.splitlines()[1::2])   # three characters a column


def test_gap_rule_in_the_driver(exe, tmp_path, wag):
    """5 taxa: two carry a block of 12 residues the other three lack, one of those three a block of its own.  Whatever tree is
    estimated, a column one taxon alone holds has no ancestor, a column every taxon holds has all of them, and the nodes present at
    a column of the shared block are those on the path between its two holders."""
    rng = np.random.default_rng(12)
    core = "".join(R._AA[x] for x in rng.integers(0, 20, 90))
    block = "WWHWCWWHCWWH"
    own = "PGPGPGPGPGPG"
    mutate = lambda s, seed: "".join(ch if q > 0.08 else R._AA[int(x)] for ch, q, x in zip(s, np.random.default_rng(seed).random(len(s)), np.random.default_rng(seed + 1).integers(0, 20, len(s))))
    seqs = [mutate(core[:45], 1) + block + mutate(core[45:], 2), mutate(core[:45], 3) + block + mutate(core[45:], 4), mutate(core, 5), mutate(core[:20], 6) + own + mutate(core[20:], 7),
            mutate(core, 8)]
    fa = str(tmp_path / "gaps.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta([("A" + s[1:]) if s[0] == "M" else s for s in seqs]))
    r = run_a(exe, fa, tmp_path, "gaps", ["-i", "0"])
    want, names, parent, rows, present = check_files(r, "aa", wag)
    holders = (rows != -1).sum(axis=0)
    assert (holders == 1).sum() >= 8 and (holders == 2).sum() >= 8 and (holders == 5).sum() >= 40
    assert not present[:, holders == 1].any() and present[:, holders == 5].all()
    kids = R.children_of(parent)
    below = lambda v: {v} if v < 5 else set().union(*[below(c) for c in kids[v]])
    for s in np.flatnonzero(holders == 2):
        a, b = np.flatnonzero(rows[:, s] != -1)
        on_path = [len(below(v) & {a, b}) == 1 or (a in below(v) and b in below(v) and all(len(below(c) & {a, b}) < 2 for c in kids[v])) for v in range(5, len(parent))]
        assert np.array_equal(present[:, s], np.array(on_path)), s
    anc = r.anc.splitlines()[1::2]
    assert all(("-" in line) == (not present[k].all()) for k, line in enumerate(anc))
