"""`--ml_ancestral_joint`, `--ml_ancestral_joint_sites` and `--ml_ancestral_samples` through the CPU oracle driver (pgmsa_oracle:
Backend::tree_ancestral_joint's and Backend::tree_ancestral_sample's defaults, the host loops), and the pieces below them:
  - tests/treelik_joint_ref.py itself against brute force (every assignment of the inner nodes' states enumerated): the joint
    assignment, its probability, and the sampler's counts;
  - the joint and the marginal reconstruction are different things;
  - tree_ancestral_joint_host and tree_ancestral_sample_host in a stand-alone program (tests/native/treelik_joint_test.cpp), its %a
    output equal to the statement bit for bit; built once plainly and once under AddressSanitizer and UBSan;
  - the driver: refusals, every other output unchanged, the stats keys, the three files against the statement on the written tree and
    the written FASTA."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_util as bu
import gen
import mldist_general_ref as M
import test_cpu_mlancestral as TA
import test_cpu_mlgamma as TG
import test_cpu_mltree as TM
import treelik_anc_ref as A
import treelik_joint_ref as J
import treelik_rates_ref as G
import treelik_ref as R
from treelik_sources import TREELIK_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOINT_HOST_SOURCES = TREELIK_HOST_SOURCES + ("treelik_joint.cpp",)   # what tests/native/treelik_joint_test.cpp links


# ---- the statement against brute force ---------------------------------------------------------------------------------------------------
def enumerate_column(dim, nleaves, parent, rows, pi, mats, s):
    """p[x] for every assignment x of the inner nodes' states (an array of shape (dim,) * ninner, axis v - nleaves the state of inner
    node v): pi[x_root] times one entry per edge, a leaf without a state the sum of its row.  mats[e][i, j]: parent state i -> child j."""
    nnodes = len(parent)
    ninner, root = nnodes - nleaves, nnodes - 1
    grid = np.indices((dim,) * ninner)
    p = pi[grid[root - nleaves]]
    for v in range(root):
        up = grid[int(parent[v]) - nleaves]
        if v >= nleaves:
            p = p * mats[v][up, grid[v - nleaves]]
        else:
            p = p * (mats[v].sum(axis=1)[up] if rows[v, s] < 0 else mats[v][up, rows[v, s]])
    return p


def brute_case(tree, ncat, seed):
    """A seeded case of 4 states on a small tree with scipy's matrices, columns with gaps and -2 among them, and per column the
    enumeration p[c][x] of every category."""
    from scipy.linalg import expm
    dim = 4
    rng = np.random.default_rng(seed)
    nleaves, parent = {"three": (3, R.caterpillar(3)), "tri": (5, R.trifurcating(5)), "five": (5, R.balanced(5))}[tree]
    nedges = len(parent) - 1
    Q = M.random_generator(dim, 40 + seed)   # (not reversible)
    pi = rng.dirichlet(np.ones(dim) * 3)
    lengths = rng.uniform(0.05, 0.6, nedges)
    ncols = 12
    rows = rng.integers(0, dim, (nleaves, ncols)).astype(np.int8)
    rows[0, 1] = -1; rows[:, 2] = -1; rows[nleaves - 1, 3] = -2
    rates, w = (np.array([1.0]), np.array([1.0])) if ncat == 1 else (np.array([0.3, 1.9]), np.array([0.35, 0.65]))
    P = G.matrices(Q, lengths, rates, derivs=False)
    mats = [[expm(Q * r * t) for t in lengths] for r in rates]
    p = [[enumerate_column(dim, nleaves, parent, rows, pi, mats[c], s) for c in range(ncat)] for s in range(ncols)]
    return dict(dim=dim, nleaves=nleaves, parent=parent, rows=rows, pi=pi, w=w, P=P, ncat=ncat, tree=tree), p


BRUTE = [(tree, ncat) for tree in ("three", "five", "tri") for ncat in (1, 2)]
BRUTE_SEED = 5   # (every column of every case has a best assignment clear of the second: printed below)


@pytest.mark.parametrize("tree,ncat", BRUTE)
def test_joint_against_brute_force(tree, ncat):
    """The statement's assignment is the enumeration's arg-max under the enumeration's most probable category on every column whose two
    best enumerated values are further apart than rounding (1e-9 relative; asserted: at least 90 % of the columns, measured: all of
    them), and joint_l 2^(-256 joint_k) is the enumeration's maximum.  Measured here: the largest relative difference over the six cases
    is 4.3e-16 (two ulps: the enumeration multiplies the same entries in another order); asserted: ten times that, 4.3e-15."""
    case, p = brute_case(tree, ncat, BRUTE_SEED)
    got = J.evaluate(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"])
    ncols, ninner = case["rows"].shape[1], len(case["parent"]) - case["nleaves"]
    assert np.all(got["joint_k"] == 0) and np.all(got["site_k"] == 0)
    clear, worst = 0, 0.0
    for s in range(ncols):
        share = np.array([case["w"][c] * p[s][c].sum() for c in range(ncat)])
        assert abs(share.sum() - got["site_l"][s]) <= 1e-12 * got["site_l"][s]
        c = int(np.argmax(share))
        assert got["cat"][s] == c   # (the categories' shares are far apart in these cases)
        flat = np.sort(p[s][c].reshape(-1))
        top, second = flat[-1], flat[-2]
        worst = max(worst, abs(got["joint_l"][s] - top) / top)
        if top - second > 1e-9 * top:
            clear += 1
            assert tuple(got["joint_state"][:, s]) == np.unravel_index(np.argmax(p[s][c]), p[s][c].shape), s
        assert got["joint_state"].shape == (ninner, ncols)
    print("%s, %d categories: %d of %d columns clear, largest relative difference of joint_l %.3g" % (tree, ncat, clear, ncols, worst))
    assert clear >= 0.9 * ncols
    assert worst <= 4.3e-15


# ---- the joint and the marginal reconstruction are different things -------------------------------------------------------------------------
def test_joint_differs_from_marginal():
    """Pinned: on the seeded case of 4 states, 33 columns, the balanced tree of 8 leaves and one category some (node, column) has another
    state in the joint assignment than in the marginal reconstruction; and on the enumerated five-leaf case the joint assignment is at
    least as probable as the assignment the marginal arg-maxes make, strictly more where they differ."""
    key = (4, 33, "balanced8", 1)
    joint, marg = J.make_case(*key)["want"], A.make_case(*key)["want"]
    differ = joint["joint_state"] != marg["anc_state"]
    print("%d of %d (node, column) pairs differ" % (differ.sum(), differ.size))
    assert differ.any() and not differ.all()
    case, p = brute_case("five", 1, BRUTE_SEED)
    args = (case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"])
    j, m = J.evaluate(*args)["joint_state"], A.evaluate(*args)["anc_state"]
    for s in range(case["rows"].shape[1]):
        pj, pm = p[s][0][tuple(j[:, s])], p[s][0][tuple(m[:, s])]
        assert pj >= pm and (pj > pm or tuple(j[:, s]) == tuple(m[:, s])), s


@pytest.mark.parametrize("key", [(4, 33, "balanced8", 1), (20, 17, "balanced8", 1), (61, 33, "trifurcating", 1), (4, 33, "three", 1)])
def test_one_category_joint_value_is_never_above_the_likelihood(key):
    """ncat == 1: the probability of the column with its best assignment is one term of the sum that site_l is."""
    want = J.make_case(*key)["want"]
    lj, ll = R.site_lnl(want["joint_l"], want["joint_k"]), R.site_lnl(want["site_l"], want["site_k"])
    assert np.all(lj <= ll + 1e-12) and np.all(want["cat"] == 0) and np.all(want["joint_state"] >= 0)


# ---- the sampler against the enumeration ----------------------------------------------------------------------------------------------
SAMPLER_N, SAMPLER_SEED = 20000, 3   # (a seed for which the statement passes: of the seeds 1 .. 4 the bound holds for 3 and 4; with 1 a cell of
#                                        N p = 0.03 holds 2 samples and with 2 a cell of N p = 0.59 holds 6, both what 6144 cells of Poisson counts bring about)


@pytest.fixture(scope="module")
def sampler():
    case, p = brute_case("five", 2, BRUTE_SEED)
    got = J.sample(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], SAMPLER_N, SAMPLER_SEED)
    return case, p, got


def within(count, p, N):
    return np.abs(count - N * p) <= 5 * np.sqrt(N * p * (1 - p)) + 1


def test_sampler_counts_of_full_assignments(sampler):
    """20000 samples of the five-leaf case with two categories: the count of every (category, assignment) of a column against its
    exact posterior p from the enumeration, |count - N p| <= 5 sqrt(N p (1 - p)) + 1."""
    case, p, got = sampler
    N, ncols, dim, ninner = SAMPLER_N, case["rows"].shape[1], case["dim"], 4
    assert np.all(got["samp_cat"] < 2) and np.all(got["samp_state"] >= 0)
    for s in range(ncols):
        exact = np.array([case["w"][c] * p[s][c] for c in range(2)])
        exact = exact / exact.sum()
        code = got["samp_cat"][s].astype(np.int64)
        for v in range(ninner):
            code = code * dim + got["samp_state"][v, s]
        count = np.bincount(code, minlength=2 * dim ** ninner).reshape(exact.shape)
        assert count.sum() == N and np.all(within(count, exact, N)), s


def test_sampler_node_frequencies(sampler):
    """... and the per-node frequencies against anc_post of the marginal statement, under the same bound."""
    case, _, got = sampler
    marg = A.evaluate(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"])
    for v in range(4):
        for s in range(case["rows"].shape[1]):
            count = np.bincount(got["samp_state"][v, s], minlength=case["dim"])
            assert np.all(within(count, marg["anc_post"][v, s], SAMPLER_N)), (v, s)
    for s in range(case["rows"].shape[1]):
        assert np.all(within(np.bincount(got["samp_cat"][s], minlength=2), marg["post"][:, s], SAMPLER_N)), s


def test_sampler_does_not_depend_on_the_cut(sampler):
    case, _, got = sampler
    args = (case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"])
    a, b = J.sample(*args, 137, SAMPLER_SEED), J.sample(*args, SAMPLER_N - 137, SAMPLER_SEED, first_sample=137)
    assert R.same_bits(np.concatenate([a["samp_cat"], b["samp_cat"]], axis=1), got["samp_cat"])
    assert R.same_bits(np.concatenate([a["samp_state"], b["samp_state"]], axis=2), got["samp_state"])
    other = J.sample(*args, 137, SAMPLER_SEED + 1)
    assert not R.same_bits(other["samp_state"], a["samp_state"])


def test_uniforms_are_splitmix64():
    """The first outputs of splitmix64 seeded with 0 (Vigna's reference values) are the draws 0, 1, 2 of seed 0, and u keeps the top 53
    bits."""
    z = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = J.uniforms(0, np.arange(3, dtype=np.uint64))
    assert u.tolist() == [(x >> 11) * 2.0 ** -53 for x in z]
    assert np.all(J.uniforms(2 ** 64 - 1, np.arange(1000, dtype=np.uint64)) < 1.0)


def test_pick_rule():
    q = np.array([[0.0, 0.25, 0.0, 0.5, 0.25, 0.0]])
    pick = lambda u, qq=q: int(J.pick(qq, np.array([u]))[0])
    assert [pick(u) for u in (0.0, 0.2499, 0.25, 0.7499, 0.75, 1.0 - 2.0 ** -53)] == [1, 1, 3, 3, 4, 4]
    assert pick(0.5, np.zeros((1, 4))) == -1                                   # T == 0.0
    assert pick(0.5, np.array([[0.0, float("nan"), 0.5, 0.0]])) == 2           # no c > target: the largest j with q_j > 0
    assert pick(0.5, np.array([[float("nan"), float("nan")]])) == -1           # ... and none
    # (with finite weights the fallback is never reached: u <= 1 - 2^-53, so u T rounds to a value below T, and c ends as T)
    for T_ in (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 3.0, 2.0 ** -1000):
        assert (1.0 - 2.0 ** -53) * T_ < T_
    assert pick(1.0 - 2.0 ** -53, np.array([[1.0, 2.0 ** -52, 0.0]])) == 1


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------------
def tie_case():
    """((0,1)3,2)4 with every entry of P_0, P_1, P_2 0.25, every row of P_3 (1/8, 3/8, 3/8, 1/8) (columns 1 and 2 equal) and pi the same:
    F_3 is constant, so states 1 and 2 of node 3 hold the maximum exactly, and so do states 1 and 2 of the root.  The smaller index wins."""
    row = np.array([0.125, 0.375, 0.375, 0.125])
    X = np.full((4, 1, 4, 4), 0.25)
    X[3, 0] = row[None, :]
    return dict(dim=4, nleaves=3, parent=R.caterpillar(3), rows=np.array([[0, -1, 3, -2], [1, -1, 3, 2], [2, 0, -1, 1]], np.int8), pi=row, w=np.array([1.0]), P=R.pack(X),
                tree="tie", ncat=1)


def degenerate_case(ncat):
    """((0,1)3,2)4 with identity matrices in category 0.  Column 0: leaves 0 and 1 disagree; column 1: they agree and leaf 2 disagrees;
    column 2: all agree; column 3: leaf 2 is missing.  Columns 0 and 1 are impossible under category 0: joint_l == 0.0 and every state
    is -1 with one category; with a second, row-stochastic category that one is the column's."""
    rng = np.random.default_rng(9)
    X = [np.stack([np.eye(4)] * 4)[:, None]]
    if ncat == 2:
        P1 = rng.uniform(0.01, 1.0, (4, 4, 4))
        X.append((P1 / P1.sum(axis=2, keepdims=True))[:, None])
    return dict(dim=4, nleaves=3, parent=R.caterpillar(3), rows=np.array([[0, 2, 1, 3], [1, 2, 1, 3], [0, 3, 1, -1]], np.int8), pi=np.array([0.1, 0.2, 0.3, 0.4]),
                w=np.full(ncat, 1.0 / ncat), P=np.concatenate([R.pack(x) for x in X]), tree="degenerate", ncat=ncat)


def test_ties_go_to_the_first_index():
    want = J.with_want(tie_case())["want"]
    assert np.all(want["joint_state"] == 1) and np.all(want["cat"] == 0)
    assert want["joint_l"].tolist() == [0.375 * 0.375 * 0.0625 * 0.25, 0.375 * 0.375 * 0.25, 0.375 * 0.375 * 0.0625, 0.375 * 0.375 * 0.0625]


def test_degenerate_columns():
    one = J.with_want(degenerate_case(1))["want"]
    assert one["joint_l"].tolist() == [0.0, 0.0, 0.2, 0.4] and one["joint_state"].T.tolist() == [[-1, -1], [-1, -1], [1, 1], [3, 3]]
    two = J.with_want(degenerate_case(2))["want"]
    assert two["cat"][:2].tolist() == [1, 1] and np.all(two["joint_state"] >= 0) and np.all(two["joint_l"] > 0)
    c = degenerate_case(1)
    s = J.sample(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"], 70, 3)
    assert np.all(s["samp_cat"][:2] == 255) and np.all(s["samp_state"][:, :2] == -1)       # post is 0 / 0 there: no category, no state
    assert np.all(s["samp_cat"][2:] == 0) and np.all(s["samp_state"][:, 2] == 1) and np.all(s["samp_state"][:, 3] == 3)
    c = degenerate_case(2)
    s = J.sample(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"], 70, 3)
    assert np.all(s["samp_cat"][:2] == 1) and np.all(s["samp_state"] >= 0) and set(s["samp_cat"][2].tolist()) == {0, 1}


# ---- the host loops, stand-alone ---------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_mljoint.py, which takes these lists from here: the host loops run every one of them.
DIMS = (4, 20, 61, 64)
GRID = [(dim, ncols, "balanced8", ncat) for dim in DIMS for ncat in (1, 4) for ncols in (1, 17, 33)]
OTHER_TREES = [(dim, 33, tree, 4) for dim in (4, 20, 64) for tree in ("two", "three", "balanced24", "trifurcating")]
MANY_COLUMNS = (4, 300, "balanced8", 4)
MIXED_SCALING = (4,)
VARYING_CATEGORY = (4, 33, "balanced8", 4)   # (its first 16 columns, one workgroup of the max pass, hold more than one category)
SMALL_VALID = (4, 15, "balanced8", 2)        # what the rejections change
JOINT_CASES = list(dict.fromkeys(GRID + OTHER_TREES + [MANY_COLUMNS, SMALL_VALID]))
SAMPLE_KEYS = [(dim, 17, "balanced8", ncat) for dim in (4, 20, 64) for ncat in (1, 4)]
SAMPLE_COUNTS, SAMPLE_SEEDS, SAMPLE_FIRSTS = (1, 64, 65, 130), (1, 0xDEADBEEFCAFEF00D), (0, 7)
NATIVE_DRAWS = [(130, SAMPLE_SEEDS[0], 0), (65, SAMPLE_SEEDS[1], 7)]   # (nsamp, seed, first_sample) of the stand-alone program


def hand_cases():
    return [tie_case(), degenerate_case(1), degenerate_case(2)]


def _case_bytes(c, nsamp=0, first=0, seed=0, which=1, **kw):
    d = dict(c); d.update(kw)
    nnodes = d.get("nnodes", len(d["parent"]))
    head = np.array([d["dim"], d["nleaves"], nnodes, d["rows"].shape[1], d["ncat"], nsamp, which], np.int32)
    parts = [head, np.array([first, seed], np.uint64), np.asarray(d["parent"], np.uint32), np.asarray(d["rows"], np.int8), np.asarray(d["pi"], np.float64),
             np.asarray(d["w"], np.float64), np.asarray(d["P"], np.float64)]
    return b"".join(np.ascontiguousarray(x).tobytes() for x in parts)


def _bad_cases():
    """What both host statements refuse, each a change to one small valid case; then no sample at all."""
    c = J.make_case(*SMALL_VALID)
    bad = []
    for ncat in (0, 17):
        bad.append(_case_bytes(c, 3, which=3, ncat=ncat, w=np.full(ncat, 0.5), P=np.tile(c["P"][:len(c["P"]) // 2], ncat)))
    for v in (0.0, -0.5, float("nan"), float("inf")):
        bad.append(_case_bytes(c, 3, which=3, w=np.array([0.5, v])))
    for b in TM._bad_cases():
        bad.append(_case_bytes(c, 3, which=3, parent=b["parent"], rows=b["rows"]))
    return bad, _case_bytes(c, 0, which=2)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """The stand-alone program built twice and run on the cases: {build: stdout lines}."""
    d = tmp_path_factory.mktemp("joint_native")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    src = [os.path.join(ROOT, "tests", "native", "treelik_joint_test.cpp")] + [os.path.join(host, f) for f in JOINT_HOST_SOURCES]
    joint = [J.make_case(*k) for k in JOINT_CASES] + [J.make_mixed_scaling_case(*MIXED_SCALING)] + [J.with_want(c) for c in hand_cases()]
    drawn = [(J.make_case(*k), k, draw) for k in SAMPLE_KEYS for draw in NATIVE_DRAWS] + [(c, c["tree"] + str(c["ncat"]), (70, 3, 0)) for c in hand_cases()]
    bad, no_sample = _bad_cases()
    path = str(d / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(joint) + len(drawn) + len(bad) + 1], np.int32).tobytes())
        for c in joint:
            f.write(_case_bytes(c))
        for c, _, (nsamp, seed, first) in drawn:
            f.write(_case_bytes(c, nsamp, first, seed, which=2))
        for blob in bad:
            f.write(blob)
        f.write(no_sample)
    # (-fno-sanitize=vptr: as tests/test_cpu_mltree.py, the unit holds Backend's virtual defaults without the drivers' backends)
    flags = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=vptr", "-fno-sanitize-recover=undefined"]}
    builds = {name: subprocess.Popen(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-I", host, "-o", str(d / ("joint_test_" + name))] + extra + src + ["-ldl"])
              for name, extra in flags.items()}
    for name in flags:
        assert builds[name].wait(timeout=600) == 0, name
    out = {}
    for name in flags:
        r = subprocess.run([str(d / ("joint_test_" + name)), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.endswith("ok %d cases\n" % (len(joint) + len(drawn) + len(bad) + 1)), r.stdout[-500:] + r.stderr[-2000:]
        out[name] = r.stdout.splitlines()
    return SimpleNamespace(joint=joint, drawn=drawn, bad=bad, lines=out)


def _floats(text):
    return np.array([float.fromhex(x) for x in text.split()])


def _ints(text, t):
    return np.array([int(x) for x in text.split()], np.int64).astype(t)


def _site_values(lines, want, what):
    assert R.same_bits(_floats(lines[0]), want["site_l"]), what
    assert np.array_equal(_ints(lines[1], np.int32), want["site_k"]), what
    assert R.same_bits(_floats(lines[2]).reshape(want["post"].shape), want["post"]), what


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_loops_equal_the_statements(native, build):
    lines = native.lines[build]
    at = 0
    for k, c in enumerate(native.joint):
        what, want = (build, "joint", k, c["dim"], c["tree"], c["ncat"]), c["want"]
        _site_values(lines[at:at + 3], want, what)
        assert R.same_bits(_ints(lines[at + 3], np.uint8), want["cat"]), what
        assert R.same_bits(_ints(lines[at + 4], np.int8).reshape(want["joint_state"].shape), want["joint_state"]), what
        assert R.same_bits(_floats(lines[at + 5]), want["joint_l"]), what
        assert np.array_equal(_ints(lines[at + 6], np.int32), want["joint_k"]), what
        at += 7
    for c, key, (nsamp, seed, first) in native.drawn:
        what = (build, "sample", key, nsamp, seed, first)
        want = J.samples_of(c, nsamp, seed, first, key=key)
        _site_values(lines[at:at + 3], want, what)
        assert R.same_bits(_ints(lines[at + 3], np.uint8).reshape(want["samp_cat"].shape), want["samp_cat"]), what
        assert R.same_bits(_ints(lines[at + 4], np.int8).reshape(want["samp_state"].shape), want["samp_state"]), what
        at += 5
    rejected = lines[at:at + 2 * len(native.bad)]
    assert len(rejected) == 2 * len(native.bad) and all(line.startswith("rejected tree likelihood:") for line in rejected), rejected
    assert lines[at + 2 * len(native.bad)] == "rejected tree ancestral sample: no sample"
    assert len(lines) == at + 2 * len(native.bad) + 2


def test_the_cases_reach_what_they_are_for():
    mixed = J.make_mixed_scaling_case(*MIXED_SCALING)["want"]
    assert np.any(mixed["joint_k"] > 0) and np.any(mixed["joint_k"] != mixed["site_k"])   # (the maxima fall below 2^-256 where the sums do not)
    assert len(set(J.make_case(*VARYING_CATEGORY)["want"]["cat"][:16].tolist())) > 1


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def run_j(exe, fa, d, tag, opts=(), joint=True, sites=True, samples=3, seed=None, env=None):
    p = {k: os.path.join(str(d), "%s.%s" % (tag, k)) for k in ("joint", "jsites", "samples", "rates")}
    extra = (["--ml_ancestral_joint", p["joint"]] if joint else []) + (["--ml_ancestral_joint_sites", p["jsites"]] if joint and sites else [])
    if samples:
        extra += ["--ml_ancestral_samples", str(samples), "--ml_ancestral_samples_out", p["samples"]] + (["--ml_ancestral_samples_seed", str(seed)] if seed is not None else [])
    if "--ml_gamma" in opts:
        extra += ["--ml_rates", p["rates"]]
    r = TM.run_ml(exe, fa, d, tag, list(opts) + extra, env=env)
    for k in p:
        setattr(r, k, open(p[k]).read() if os.path.exists(p[k]) else None)
    return r


def check_files(run, kind, model, K=0, nsamp=3, seed=1):
    """The three files against the statements on the written tree (--ml_tree: the topology and the lengths), the written alpha and the
    written FASTA.  The states, the categories and the gap rule must match exactly.  The newick's 6 digits move a length t by up to
    5e-6 t, so an entry of P(r_c t_e) moves by at most (relative) eps_e = max |r_c (Q P)_ab / P_ab| 5e-6 t_e (tests/test_cpu_mlancestral.py:
    check_files); joint_l is a product of one entry (or one row sum) of every edge's matrix, all positive, times pi, and the maximum of
    functions that each move by at most that moves by no more: |ln joint_l - the statement's| <= sum_e eps_e to first order; the bound
    takes twice that plus 1e-9 relative (the matrices of the two sides: scipy's expm against the driver's)."""
    from scipy.linalg import expm
    Q, pi = model
    dim = len(pi)
    sym = TA.symbols_of(kind)
    width = len(sym[0])
    names, parent, lengths = R.from_newick(run.tree)
    nleaves, ninner = len(names), len(parent) - len(names)
    rows = R.rows_of(TM.parse_fasta(run.stdout), names, kind)
    ncols = rows.shape[1]
    if K:
        alpha, rates, _ = TG.parse_rates(run.rates)
        rates, w = G.gamma_rates(alpha, K), G.weights_of(K)
    else:
        rates, w = np.array([1.0]), np.array([1.0])
    P = G.matrices(Q, lengths, rates, derivs=False)
    want = J.evaluate(dim, nleaves, parent, rows, pi, w, P)
    present = A.presence(nleaves, parent, rows)
    text = lambda states, k: "".join(sym[states[s]] if present[k, s] and states[s] >= 0 else "-" * width for s in range(ncols))
    recs = run.joint.splitlines()
    assert recs == [x for k in range(ninner) for x in (">N%d" % (k + 1), text(want["joint_state"][k], k))]
    eps = np.zeros(len(lengths))
    for e, t in enumerate(lengths):
        for r in rates:
            Pm = expm(Q * r * t)
            eps[e] = max(eps[e], float(np.max(np.abs(r * (Q @ Pm) / Pm))) * 5e-6 * t)
    ref = R.site_lnl(want["joint_l"], want["joint_k"])
    bound = 2 * float(eps.sum()) + 1e-9 * np.abs(ref) + 1e-12
    lines = run.jsites.splitlines()
    assert len(lines) == ncols + 1 and lines[0].startswith("lnJ ")
    total, worst = 0.0, 0.0
    for s in range(ncols):
        col, cat, value = lines[s + 1].split("\t")
        assert int(col) == s + 1 and int(cat) == int(want["cat"][s]) + 1 and "%.17g" % float(value) == value
        worst = max(worst, abs(float(value) - ref[s]) / bound[s])
        total = total + float(value)
    print("largest |lnJ column difference| over its bound: %.3g" % worst)
    assert worst <= 1.0 and lines[0] == "lnJ %.17g" % total
    if not K:   # (one category: a term of the sum that site_l is; under --ml_gamma joint_l carries no weight and may exceed the mixture's value)
        assert np.all(ref <= R.site_lnl(want["site_l"], want["site_k"]) + 1e-12)
    if nsamp:
        drawn = J.sample(dim, nleaves, parent, rows, pi, w, P, nsamp, seed)
        recs = run.samples.splitlines()
        assert recs == [x for n in range(nsamp) for k in range(ninner) for x in (">N%d/%d" % (k + 1, n + 1), text(drawn["samp_state"][k, :, n], k))]
    return want, rows, present


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlj_fams")
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
    joint = ["--ml_ancestral_joint", p("joint")]
    samples = ["--ml_ancestral_samples", "3", "--ml_ancestral_samples_out", p("samples")]
    need_ml = "--ml_ancestral_joint and --ml_ancestral_samples need --ml_tree"
    count = "--ml_ancestral_samples takes a number of samples from 1 to 1000"
    seed = "--ml_ancestral_samples_seed takes a whole number from 0 to 18446744073709551615"
    cases = [
        (joint + [fa], need_ml),
        (["--ml_ancestral_joint_sites", p("js"), fa], need_ml),
        (samples + [fa], need_ml),
        (["--ml_ancestral_samples_out", p("samples"), fa], need_ml),
        (["--ml_ancestral_samples_seed", "4", fa], need_ml),
        (ml + ["--ml_ancestral_joint_sites", p("js"), fa], "--ml_ancestral_joint_sites needs --ml_ancestral_joint"),
        (ml + ["--ml_ancestral_samples", "3", fa], "--ml_ancestral_samples and --ml_ancestral_samples_out need each other"),
        (ml + ["--ml_ancestral_samples_out", p("samples"), fa], "--ml_ancestral_samples and --ml_ancestral_samples_out need each other"),
        (ml + joint + ["--ml_ancestral_samples_seed", "4", fa], "--ml_ancestral_samples_seed needs --ml_ancestral_samples"),
        (ml + joint + samples + ["--batch", lst], "--batch cannot be combined with --ml_tree"),
        (joint + ["--batch", lst], "--batch cannot be combined with --ml_tree"),
        (["--ml_ancestral_samples_seed", "4", "--batch", lst], "--batch cannot be combined with --ml_tree"),
        # what the tests of the older flags pin stays as it is for its combination of flags, with the new ones beside them
        (joint + ["--ml_sites", p("sites"), fa], "--ml_sites, --ml_rounds and --ml_epsilon need --ml_tree"),
        (joint + ["--ml_gamma", "4", fa], "--ml_gamma, --ml_alpha and --ml_rates need --ml_tree"),
        (joint + ["--ml_ancestral", p("anc"), fa], "--ml_ancestral needs --ml_tree"),
        (ml + joint + ["--ml_alpha", "0.5", fa], "--ml_alpha and --ml_rates need --ml_gamma"),
        (ml + joint + ["--ml_ancestral_probs", p("ap"), fa], "--ml_ancestral_tree and --ml_ancestral_probs need --ml_ancestral"),
        (ml + joint + ["--ml_gamma", "1", fa], "from 2 to 16"),
        (ml + joint + samples + ["-W", fa], "--ml_tree cannot be combined with -W"),
        (ml + joint + samples + ["-r", fa], "--ml_tree cannot be combined with -r"),
        (ml + joint + [fams[2]], "at least 3 sequences"),
        (ml + samples + [fams[2]], "at least 3 sequences"),
    ]
    for n in ("0", "1001", "-1", "x", "3.5", "", "1e2"):
        cases.append((ml + ["--ml_ancestral_samples", n, "--ml_ancestral_samples_out", p("samples"), fa], count))
    for s in ("-1", "abc", "1e3", "", "1.5", "18446744073709551616", "+4"):
        cases.append((ml + samples + ["--ml_ancestral_samples_seed", s, fa], seed))
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [q for q in os.listdir(str(tmp_path)) if q.startswith("never") or q == "b.out"]
        assert left == [], (args, left)
    ok = run_j(exe, fa, tmp_path, "edge", ["-i", "0"], joint=False, samples=1000, seed=18446744073709551615)   # the ends of both ranges
    assert ok.samples.count(">") == 1000 * 4 and ok.joint is None


@pytest.mark.parametrize("flags", [["--ml_ancestral_joint"], ["--ml_ancestral_samples", "2", "--ml_ancestral_samples_out"]])
def test_a_leaf_with_a_node_name_is_refused(exe, tmp_path, flags):
    seqs = gen.gen(4, 60, 77)
    fa = str(tmp_path / "names.fa")
    with open(fa, "w") as f:
        for name, s in zip(["a", "N2", "b", "c"], seqs):
            f.write(">%s\n%s\n" % (name, s))
    r = subprocess.run([exe, "--fasta", "--ml_tree", str(tmp_path / "t")] + flags + [str(tmp_path / "never.out"), fa], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "N2" in r.stderr and "inner node" in r.stderr and flags[0] in r.stderr
    assert not os.path.exists(str(tmp_path / "never.out")) and not os.path.exists(str(tmp_path / "t"))   # (before the optimiser and any file)


def test_other_outputs_unchanged_and_stats(exe, fams, tmp_path):
    fa = fams[8]
    for tag, opts in (("p", []), ("g", ["--ml_gamma", "4"])):
        old = TA.run_a(exe, fa, tmp_path, "old" + tag, opts)
        assert "ml_ancestral_joint_s" not in old.stats and "ml_ancestral_samples_s" not in old.stats
        p = {k: str(tmp_path / ("new%s.%s" % (tag, k))) for k in ("joint", "jsites", "samples")}
        new = TA.run_a(exe, fa, tmp_path, "new" + tag, opts + ["--ml_ancestral_joint", p["joint"], "--ml_ancestral_joint_sites", p["jsites"], "--ml_ancestral_samples", "5",
                                                             "--ml_ancestral_samples_out", p["samples"]])
        assert (new.stdout, new.tree, new.sites, new.rates, new.anc, new.anctree, new.probs) == (old.stdout, old.tree, old.sites, old.rates, old.anc, old.anctree, old.probs)
        assert len(new.stdout) > 0 and len(new.tree) > 0 and len(new.anc) > 0 and all(os.path.getsize(q) > 0 for q in p.values())
        assert sorted(set(new.stats) - set(old.stats)) == ["ml_ancestral_joint_s", "ml_ancestral_samples_s"] and set(old.stats) <= set(new.stats)
        assert new.stats["ml_ancestral_joint_s"] > 0 and new.stats["ml_ancestral_samples_s"] > 0 and new.stats["ml_kernel_ms"] == 0
        for k in ("ml_lnl", "ml_lnl_start", "ml_rounds", "ml_evaluations"):
            assert new.stats[k] == old.stats[k], k
        one = run_j(exe, fa, tmp_path, "one" + tag, opts, sites=False, samples=0)   # each flag alone, and none needs --ml_ancestral
        assert one.joint == open(p["joint"]).read() and one.jsites is None and one.samples is None
        assert "ml_ancestral_samples_s" not in one.stats and "ml_ancestral_s" not in one.stats and one.stats["ml_ancestral_joint_s"] > 0
        two = run_j(exe, fa, tmp_path, "two" + tag, opts, joint=False, samples=5)
        assert two.samples == open(p["samples"]).read() and two.joint is None and "ml_ancestral_joint_s" not in two.stats
        for switch in ("PGM_HOST_TREELIK", "PGM_DEVICE_TREELIK"):   # (this driver's backend has the default bodies: the host loops either way)
            h = run_j(exe, fa, tmp_path, switch + tag, opts, samples=5, env=dict(os.environ, **{switch: "1"}))
            assert (h.joint, h.jsites, h.samples) == (open(p["joint"]).read(), open(p["jsites"]).read(), open(p["samples"]).read())


def test_samples_depend_on_the_seed_alone(exe, fams, tmp_path):
    fa = fams[8]
    a = run_j(exe, fa, tmp_path, "a", ["-i", "0"], joint=False, samples=4)
    b = run_j(exe, fa, tmp_path, "b", ["-i", "0"], samples=4, seed=1)                       # the default seed, the joint files beside it
    c = run_j(exe, fa, tmp_path, "c", ["-i", "0"], joint=False, samples=7, seed=1)          # more samples: the first four are the same
    d = run_j(exe, fa, tmp_path, "d", ["-i", "0"], joint=False, samples=4, seed=2)
    assert a.samples == b.samples and len(a.samples) > 0
    assert c.samples.startswith(a.samples) and c.samples.count(">") == 7 * a.samples.count(">") // 4
    assert d.samples != a.samples and d.samples.count(">") == a.samples.count(">")
    assert [line for line in d.samples.splitlines() if line.startswith(">")] == [line for line in a.samples.splitlines() if line.startswith(">")]


@pytest.mark.parametrize("n,opts", [(5, []), (5, ["--ml_gamma", "4"]), (13, []), (8, ["--ml_gamma", "4", "--ml_alpha", "0.7"])])
def test_files_aa(exe, fams, tmp_path, wag, n, opts):
    """Amino acids with and without --ml_gamma; the family of 5 has a re-inserted start column (an X where M was stripped)."""
    r = run_j(exe, fams[n], tmp_path, "f", ["-i", "0"] + opts)
    want, rows, present = check_files(r, "aa", wag, 4 if opts else 0)
    full = (rows != -1).all(axis=0)
    assert full.any() and present[:, full].all()
    if opts:
        assert len(set(want["cat"].tolist())) > 1


def test_files_behind_the_search(exe, fams, tmp_path, wag):
    """--ml_search: the files describe the tree the run ends with."""
    r = run_j(exe, fams[8], tmp_path, "s", ["-i", "0", "--ml_search", "3"])
    check_files(r, "aa", wag)
    assert "ml_search_s" in r.stats


def test_dna_custom_model_and_codon(exe, fams, tmp_path):
    hky = R.custom(fams["hky"], 4)
    fa = [f for f in fams["dna"] if len(R.read_fasta(f)) >= 3][0]
    r = run_j(exe, fa, tmp_path, "dna", ["--dna", "--custom_model", fams["hky"]], seed=11)
    check_files(r, "dna", hky, seed=11)
    ecm = R.shipped("ecm.qmat")
    r = run_j(exe, fams["codon"][1], tmp_path, "cod", ["--codon", "--ml_rounds", "3", "--ml_gamma", "2"], samples=2)
    want, rows, present = check_files(r, "codon", ecm, 2, nsamp=2)
    assert all(len(line) == 3 * rows.shape[1] for line in r.joint.splitlines()[1::2])   # three characters a column
