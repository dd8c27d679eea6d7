"""The shapes of the tree likelihood entries (pgm_tree_likelihood, pgm_tree_likelihood_rates, pgm_tree_ancestral, pgm_tree_nni) that the
grids of tests/test_cpu_ml*.py and tests/test_gpu_ml*.py leave out: the lists of cases, and what they claim, checked on the CPU.

tests/test_gpu_treelik_shapes.py runs every list on the device; the four tests/test_cpu_ml*.py files append the NATIVE_* lists below
to the cases of their stand-alone host programs, so the host loop meets the statement on the same cases.  This file imports the
statements only (the other four import it).

A. Every kind of dim the C ABI accepts beside {4, 20, 61, 64}.  A wavefront holds spb = 64 / dim sites, one thread per (site, state);
   the sums over states run in blocks of eight and a tail.  NEW_DIMS: 1 and 2 (64 and 32 sites; the scans from 1 are empty at dim 1),
   8, 16, 32 (whole blocks, no idle lane), 7 and 9 (either side of one block), 21 and 22 (spb 3 and 2), 32 and 33 (spb 2 and 1), 3 and
   63 (one idle lane), 5.  Columns: 1, spb, spb + 1 and 4 spb + 1 (the edge of a wavefront, and one site past a workgroup of the
   candidates' kernel, which has four wavefronts).
B. The second rounds of the strided loops.  The sums kernel takes a second chunk per thread above 64 chunks of 16 = 1024 columns;
   the combine kernel a second edge per workgroup above 65535 edges; the ancestral combine kernel a second pair per workgroup above
   2^20 (node, site) pairs at one pair per wavefront (dim >= 33).  The last two are device cases only.
C. Polytomies: a node of three or four children below the root (inner or leaves), a root of five leaves, a root of three kinds of
   children."""
import numpy as np
import pytest

import treelik_anc_ref as A
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R

def ident(key):
    """A case's test id: dim, ncols, tree, then ncat or whether derivatives are asked for."""
    return "dim%d-ncols%d-%s-%s" % (key[0], key[1], key[2], ("derivs" if key[3] else "noderivs") if isinstance(key[3], bool) else "ncat%d" % key[3])


# ---- A: every kind of dim --------------------------------------------------------------------------------------------------------------
NEW_DIMS = (1, 2, 3, 5, 7, 8, 9, 16, 21, 22, 32, 33, 63)


def ncols_of(dim):
    spb = 64 // dim
    return list(dict.fromkeys((1, spb, spb + 1, 4 * spb + 1)))


DIM_SHAPES = [(dim, ncols) for dim in NEW_DIMS for ncols in ncols_of(dim)]
DIMS_PLAIN = [(dim, ncols, "balanced8", True) for dim, ncols in DIM_SHAPES]
DIMS_RATES = [(dim, ncols, "balanced8", 2) for dim, ncols in DIM_SHAPES] + [(dim, ncols, "balanced8", 16) for dim in (1, 63) for ncols in ncols_of(dim)]
DIMS_ANC = [(dim, ncols, "balanced8", 2) for dim, ncols in DIM_SHAPES]   # with anc_post
DIMS_NNI = [(dim, ncols, "balanced8", 2) for dim, ncols in DIM_SHAPES]   # all 12 candidates
SCALING_DIMS = (1, 3, 8, 33)
SCALING_PLAIN = [(dim, 64 // dim + 1, "caterpillar96", True) for dim in SCALING_DIMS]
SCALING_RATES = [(dim, 64 // dim + 1, "caterpillar96", 2) for dim in SCALING_DIMS]
NO_DERIVS = [(dim, 4 * (64 // dim) + 1, "balanced8", False) for dim in (3, 8, 33)]

# ---- B: second rounds -------------------------------------------------------------------------------------------------------------------
SUMS_NCOLS = (1024, 1025, 2049)   # 64 chunks; 65, the last of one site; 129: thread 0 takes three
SUMS_PLAIN = [(4, ncols, "balanced8", True) for ncols in SUMS_NCOLS]
SUMS_RATES = [(4, ncols, "balanced8", 2) for ncols in SUMS_NCOLS]
EDGES = (2, 2, "balanced32770", 2)   # 65538 edges: three workgroups of the combine kernel take a second one
EDGES_GRID = 65535
PAIRS_BLOCK = (33, 1021, "two", 2)   # one inner node, a prime number of columns
PAIRS_NCOLS = 2 ** 20 + 3            # (node, site) pairs at one per wavefront: three workgroups take a second one
PAIRS_GRID = 2 ** 20


def edges_case():
    """The rates case of B2 and its expectation (some ten seconds of the statement: 32769 inner nodes in a Python loop, twice);
    computed once per process.  The plain entry's expectation is not computed."""
    return G.make_case(*EDGES, plain_want=False)


def tiled(x, ncols, axis=-1):
    """x's columns (along `axis`) repeated in order up to ncols of them."""
    x = np.asarray(x)
    reps = [1] * x.ndim
    reps[axis] = -(-ncols // x.shape[axis])
    return np.ascontiguousarray(np.take(np.tile(x, reps), np.arange(ncols), axis=axis))


COLUMN_AXIS = dict(site_l=0, site_k=0, post=1, anc_state=1, anc_prob=1, anc_post=1)


def pairs_case(ncols=PAIRS_NCOLS):
    """B3: the block case's rows repeated up to ncols columns, and the block's expectation repeated the same way (the columns are
    independent: test_columns_are_independent holds the statement to it)."""
    block = A.make_case(*PAIRS_BLOCK)
    want = {k: tiled(block["want"][k], ncols, axis) for k, axis in COLUMN_AXIS.items() if k != "anc_post" or ncols < 10000}
    return dict(block, rows=tiled(block["rows"], ncols, 1), want=want)


# ---- C: polytomies ---------------------------------------------------------------------------------------------------------------------
POLY_DIMS = (3, 4, 20, 33, 61, 64)
POLY_TREES = ("inner3", "inner4", "leaves4", "star5", "mixed3")
POLY_NCOLS = 17
POLY_PLAIN = [(dim, POLY_NCOLS, tree, derivs) for tree in POLY_TREES for dim in POLY_DIMS for derivs in (True, False)]
POLY_RATES = [(dim, POLY_NCOLS, tree, 2) for tree in POLY_TREES for dim in POLY_DIMS]
POLY_ANC = list(POLY_RATES)
POLY_NNI = [(dim, POLY_NCOLS, tree, 2) for tree in POLY_TREES if tree != "star5" for dim in POLY_DIMS]   # (a star has no candidate)

# ---- what the stand-alone host programs take on top of their own lists (B2 and B3 stay out: the files would be the cost) ----------------
NATIVE_PLAIN = DIMS_PLAIN + SCALING_PLAIN + NO_DERIVS + SUMS_PLAIN + POLY_PLAIN   # (dim, ncols, tree, derivs)
NATIVE_RATES = DIMS_RATES + SCALING_RATES + SUMS_RATES + POLY_RATES              # (dim, ncols, tree, ncat), derivs on
NATIVE_ANC = DIMS_ANC + POLY_ANC                                                 # (dim, ncols, tree, ncat)
NATIVE_NNI = DIMS_NNI + POLY_NNI                                                 # (dim, ncols, tree, ncat), every candidate


# ---- the lists hold what they claim ----------------------------------------------------------------------------------------------------
def test_dims_and_columns():
    assert all(1 <= dim <= 64 and dim not in (4, 20, 61, 64) for dim in NEW_DIMS)
    assert {64 // dim for dim in NEW_DIMS} == {64, 32, 21, 12, 9, 8, 7, 4, 3, 2, 1}
    assert [dim for dim in NEW_DIMS if 64 % dim == 0] == [1, 2, 8, 16, 32] and [dim for dim in NEW_DIMS if 64 - dim * (64 // dim) == 1] == [3, 7, 9, 21, 63]
    assert ncols_of(1) == [1, 64, 65, 257] and ncols_of(3) == [1, 21, 22, 85] and ncols_of(32) == [1, 2, 3, 9] and ncols_of(33) == [1, 2, 5] == ncols_of(63)
    assert len(DIM_SHAPES) == 4 * 11 + 2 * 3 and len(DIMS_RATES) == len(DIM_SHAPES) + 4 + 3
    for lists in (NATIVE_PLAIN, NATIVE_RATES, NATIVE_ANC, NATIVE_NNI):
        assert len(set(lists)) == len(lists)


def test_thresholds():
    """The cases of B sit just past the launch caps they are about."""
    chunks = [-(-n // R.CHUNK) for n in SUMS_NCOLS]
    assert chunks == [64, 65, 129] and SUMS_NCOLS[1] % R.CHUNK == 1
    nleaves, parent = R.TREES[EDGES[2]]()
    assert (nleaves, len(parent), len(parent) - 1 - EDGES_GRID) == (32770, 65539, 3)
    kids = R.children_of(parent)
    assert all(len(k) == 2 for k in kids[nleaves:]) and all(int(p) > v for v, p in enumerate(parent[:-1]))
    nleaves, parent = R.TREES[PAIRS_BLOCK[2]]()
    assert 64 // PAIRS_BLOCK[0] == 1 and (len(parent) - nleaves) * PAIRS_NCOLS - PAIRS_GRID == 3
    assert PAIRS_NCOLS % PAIRS_BLOCK[1] not in (0, 1) and all(PAIRS_BLOCK[1] % p for p in range(2, 32))


def test_polytomy_trees():
    shape = {}
    for tree in POLY_TREES:
        nleaves, parent = R.TREES[tree]()
        kids = R.children_of(parent)
        root = len(parent) - 1
        assert int(parent[root]) == R.ROOT and all(v < int(p) <= root for v, p in enumerate(parent[:-1])) and not any(kids[:nleaves])
        assert all(len(k) >= 2 for k in kids[nleaves:])
        shape[tree] = {v: (len(kids[v]), sum(c >= nleaves for c in kids[v])) for v in range(nleaves, root + 1)}   # node: (children, inner ones)
        ncand = len(N.candidates(nleaves, parent))
        assert ncand == sum(len(kids[v]) * (len(kids[int(parent[v])]) - 1) for v in range(nleaves, root))
        assert (ncand == 0) == (tree == "star5")
    assert shape["inner3"] == {6: (3, 0), 7: (2, 1), 8: (2, 1), 9: (2, 1)}
    assert shape["inner4"] == {7: (2, 0), 8: (2, 0), 9: (4, 2), 10: (2, 1)}
    assert shape["leaves4"] == {6: (4, 0), 7: (2, 0), 8: (2, 2)}
    assert shape["star5"] == {5: (5, 0)}
    assert shape["mixed3"] == {6: (3, 0), 7: (2, 0), 8: (3, 2)}
    assert np.array_equal(R.TREES["inner3"]()[1], N.TREES["inner3"]()[1])


@pytest.mark.parametrize("tree", POLY_TREES)
def test_polytomy_equals_its_resolution_by_an_edge_of_length_zero(tree):
    """A node of more than two children is the binary node whose extra edge carries the identity matrix: the site likelihoods agree
    within 1e-12 relative (the products associate differently), here at 4 states and at 20."""
    for dim in (4, 20):
        case = R.make_case(dim, POLY_NCOLS, tree, False)
        nleaves, parent = case["nleaves"], [int(p) for p in case["parent"]]
        X = [m for m in R.unpack(case["P"], len(parent) - 1, 1, dim)]
        kids = R.children_of(case["parent"])
        # rebuild children before parents: every node with children c0, c1, c2 ... becomes ((c0, c1)x, c2)y ...
        new_parent, new_X, number = [], [], {}
        for l in range(nleaves):
            number[l] = l
            new_parent.append(None); new_X.append(X[l])
        for v in range(nleaves, len(parent)):
            below = number[kids[v][0]]
            for c in kids[v][1:-1]:
                new_parent.append(None); new_X.append(np.eye(dim)[None])
                new_parent[below] = new_parent[number[c]] = len(new_parent) - 1
                below = len(new_parent) - 1
            new_parent.append(None); new_X.append(X[v] if v < len(parent) - 1 else None)
            number[v] = len(new_parent) - 1
            new_parent[below] = new_parent[number[kids[v][-1]]] = number[v]
        new_parent[-1] = R.ROOT
        assert len(new_parent) == 2 * nleaves - 1 > len(parent)
        got = R.evaluate(dim, nleaves, np.array(new_parent, np.uint32), case["rows"], case["pi"], R.pack(np.array(new_X[:-1])), False)
        want = case["want"]
        assert np.array_equal(got["site_k"], want["site_k"])
        assert np.max(np.abs(got["site_l"] - want["site_l"]) / want["site_l"]) < 1e-12


def test_columns_are_independent():
    """What B3 rests on: the ancestral statement on three periods of the block's columns and five more equals the block's expectation
    repeated, bit for bit (anc_post among them)."""
    block = A.make_case(*PAIRS_BLOCK)
    ncols = 3 * PAIRS_BLOCK[1] + 5
    case = pairs_case(ncols)
    assert case["rows"].shape == (2, ncols) and np.array_equal(case["rows"][:, -5:], block["rows"][:, :5]) and np.array_equal(case["rows"][:, 1021:2042], block["rows"])
    got = A.evaluate(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"])
    assert sorted(case["want"]) == sorted(COLUMN_AXIS)
    for k, want in case["want"].items():
        assert R.same_bits(got[k], want), k
    assert len({bytes(c) for c in block["rows"].T.copy()}) > 500   # (the block is no repetition itself)
    assert "anc_post" not in pairs_case(20000)["want"]


def test_new_cases_are_no_degenerate_ones():
    """No NaN among the derivatives of the new dims, the caterpillars rescale on their full columns (one state included), and a
    polytomy's derivatives differ per edge."""
    for key in SCALING_PLAIN:
        case = R.make_case(*key)
        full = (case["rows"] >= 0).all(axis=0)
        assert full.any() and np.all(case["want"]["site_k"][full] > 0) and not np.any(np.isnan(case["want"]["d1"])), key
    for dim in NEW_DIMS:
        want = R.make_case(dim, 64 // dim + 1, "balanced8")["want"]
        assert not np.any(np.isnan(want["d1"])) and not np.any(np.isnan(want["d2"])) and np.all(want["site_k"] == 0), dim
    want = R.make_case(20, POLY_NCOLS, "inner4")["want"]
    assert len(set(want["d1"].tolist())) == len(want["d1"])
