"""The nearest-neighbour interchange scores of `pgmsa --ml_tree --ml_search` stated independently of the C++ and the kernels (DESIGN
3.20; include/pgm_hip.h: pgm_tree_nni), in numpy float64, vectorised over the sites only.

site_l, site_k and post are treelik_rates_ref.evaluate's without derivatives; the walk of one category is treelik_anc_ref's restated to
keep the partials U and the outside vectors O (P alone), every sum a Python loop ascending from 0.0 with one multiply and one add per
term.  The helpers around it (the candidates of a tree, the exchanged tree renumbered, bipartitions) and the seeded cases serve
tests/test_cpu_mlsearch.py and tests/test_gpu_mlsearch.py."""
import numpy as np

import treelik_anc_ref as A
import treelik_rates_ref as G
import treelik_ref as R
from treelik_ref import _apply, _dot, _rescale, children_of

ROOT = R.ROOT


def walk(dim, nleaves, parent, rows, pi, X):
    """One category: X[e][0][i, j], P alone.  Returns (L, k), the partials U[v][s, i] (the leaves' indicators among them) and the
    scaled outside vectors O[v][s, i] of the inner nodes below the root."""
    nnodes, ncols = len(parent), rows.shape[1]
    root = nnodes - 1
    kids = children_of(parent)
    states = np.arange(dim)
    U = [None] * nnodes
    for l in range(nleaves):
        U[l] = ((rows[l][:, None] < 0) | (rows[l][:, None] == states[None, :])).astype(np.float64)
    k = np.zeros(ncols, np.int32)
    for v in range(nleaves, nnodes):
        prod = None
        for c in kids[v]:
            S = _apply(X[c][0], U[c])
            prod = S if prod is None else prod * S
        U[v], hit = _rescale(prod)
        k += hit
    L = _dot(np.broadcast_to(pi, (ncols, dim)), U[root])
    O = [None] * nnodes
    for v in range(root, nleaves - 1, -1):
        base = _base(dim, ncols, pi, X, O, v, root)
        S = {c: _apply(X[c][0], U[c]) for c in kids[v]}
        for c in kids[v]:
            if c < nleaves:
                continue
            o = base
            for sib in kids[v]:
                if sib != c:
                    o = o * S[sib]
            O[c], _ = _rescale(o)
    return L, k, U, O


def _base(dim, ncols, pi, X, O, u, root):
    """B_u[s, i]: pi at the root, else sum over h ascending of O_u(h) P_u(h, i)."""
    if u == root:
        return np.broadcast_to(pi, (ncols, dim)).copy()
    base = np.zeros((ncols, dim))
    for hh in range(dim):
        base = base + O[u][:, hh][:, None] * X[u][0][hh, :][None, :]
    return base


def evaluate(dim, nleaves, parent, rows, pi, w, P, cand):
    """pgm_tree_nni.  cand: rows (v, a, c).  Returns a dict: site_l, site_k, post (ncat x ncols), rho (ncand x ncols), and per category
    the ratios cat_rho (ncat x ncand x ncols) and the counts cat_kd, cat_kn of the two trees."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    cand = np.asarray(cand, np.int64).reshape(-1, 3)
    ncat, nedges, ncols, ncand = len(w), len(parent) - 1, rows.shape[1], len(cand)
    root = len(parent) - 1
    kids = children_of(parent)
    Xall = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    post = out["post"]
    rho = np.zeros((ncand, ncols))
    cat_rho, cat_kd, cat_kn = np.zeros((ncat, ncand, ncols)), np.zeros((ncat, ncand, ncols), np.int32), np.zeros((ncat, ncand, ncols), np.int32)
    walks = []
    for k in range(ncat):
        X = R.unpack(Xall[k], nedges, 1, dim)
        L, kk, U, O = walk(dim, nleaves, parent, rows, pi, X)
        assert R.same_bits(L, out["cat_l"][k]) and np.array_equal(kk, out["cat_k"][k])   # (the same up pass)
        walks.append((X, U, O))
    for q, (v, a, c) in enumerate(cand):
        v, a, c = int(v), int(a), int(c)
        u = int(parent[v])
        assert v >= nleaves and u != ROOT and int(parent[a]) == v and int(parent[c]) == u and c != v
        mixed = np.zeros(ncols)
        for k in range(ncat):
            X, U, O = walks[k]
            S = lambda x: _apply(X[x][0], U[x])
            Rv = _base(dim, ncols, pi, X, O, u, root)
            for sib in kids[u]:
                if sib != v and sib != c:
                    Rv = Rv * S(sib)
            T = None
            for b in kids[v]:
                if b != a:
                    T = S(b) if T is None else T * S(b)
            Sa, Sc = S(a), S(c)
            vals = []
            for Sx, Sy in ((Sa, Sc), (Sc, Sa)):
                Xv, hx = _rescale(T * Sx)
                Yv, hy = _rescale(Rv * Sy)
                W = _apply(X[v][0], Xv)
                vals.append((_dot(Yv, W), hx.astype(np.int32) + hy.astype(np.int32)))
            (D, kD), (N, kN) = vals
            with np.errstate(all="ignore"):
                r = np.where(D == 0.0, 0.0, N / D)
            for n in range(int(max((kN - kD).max(), 0))):
                r = np.where(kN - kD > n, r * R.TINY, r)
            for n in range(int(max((kD - kN).max(), 0))):
                r = np.where(kD - kN > n, r * R.SCALE, r)
            cat_rho[k, q], cat_kd[k, q], cat_kn[k, q] = r, kD, kN
            mixed = mixed + post[k] * r
        rho[q] = mixed
    out.update(rho=rho, cat_rho=cat_rho, cat_kd=cat_kd, cat_kn=cat_kn)
    return out


def gain(rho):
    """treelik_nni_gain: per candidate the sum over the sites ascending of log rho (log 0 = -inf).  The logarithm is the C library's
    (math.log), as in the host code: numpy's own may differ from it in the last bit."""
    import math
    out = np.zeros(rho.shape[0])
    for q in range(rho.shape[0]):
        total = 0.0
        for x in rho[q]:
            total = total + (math.log(x) if x > 0.0 else -math.inf if x == 0.0 else math.nan)
        out[q] = total
    return out


# ---- trees -------------------------------------------------------------------------------------------------------------------------
def candidates(nleaves, parent):
    """Every candidate of a tree in the search's order: v ascending, a in child order, c in child order."""
    kids = children_of(parent)
    out = []
    for v in range(nleaves, len(parent) - 1):
        for a in kids[v]:
            for c in kids[int(parent[v])]:
                if c != v:
                    out.append((v, a, c))
    return np.array(out, np.uint32).reshape(-1, 3)


def exchanged(nleaves, parent, v, a, c):
    """The neighbour tree of candidate (v, a, c), renumbered children before parents (the leaves keep their numbers).  Returns
    (parent', old) with old[new node] = the node's number in the given tree: edge e' of the new tree has the matrices of edge old[e']."""
    p = [int(x) for x in parent]
    u = p[v]
    p[a], p[c] = u, v
    kids = [[] for _ in p]
    for x, y in enumerate(p):
        if y != ROOT:
            kids[y].append(x)
    order = list(range(nleaves))

    def post(x):
        for y in kids[x]:
            post(y)
        if x >= nleaves:
            order.append(x)

    post(len(p) - 1)
    new = {old: k for k, old in enumerate(order)}
    out = [ROOT] * len(p)
    for old, k in new.items():
        if p[old] != ROOT:
            out[k] = new[p[old]]
    return np.array(out, np.uint32), np.array(order)


inner_trifurcation = R.inner_trifurcation

TREES = dict(R.TREES)
TREES["four"] = lambda: (4, R.balanced(4))
OWN_DRAW = ("four", "inner3")   # the trees whose cases make_case draws itself (inner3 since before treelik_ref had it: its cases keep their bits)


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def make_case(dim, ncols, tree, ncat, which="all"):
    """A seeded case and its expectation, computed once per process.  The rows, pi and matrices are drawn as treelik_ref.make_case
    draws them (the trees of its table are its own cases); `which`: "all" candidates in the search's order, "root" the candidates
    whose u is the root, "one" the first alone, "shuffled" all of them in a seeded order with the first three repeated at the end."""
    key = (dim, ncols, tree, ncat, which)
    if key in _cases:
        return _cases[key]
    if tree not in OWN_DRAW:
        base = A.make_case(dim, ncols, tree, ncat)
        nleaves, parent, rows, pi, P, w = base["nleaves"], base["parent"], base["rows"], base["pi"], base["P"], base["w"]
    else:
        nleaves, parent = TREES[tree]()
        nedges = len(parent) - 1
        rng = np.random.default_rng(5000 + 1000 * dim + 7 * ncols + 13 * ncat + sum(map(ord, tree)))
        pi = rng.dirichlet(np.ones(dim) * 4)
        P0 = rng.uniform(0.01, 1.0, (ncat * nedges, dim, dim))
        P0 /= P0.sum(axis=2, keepdims=True)
        P = R.pack(P0[:, None])
        rows = rng.integers(0, dim, (nleaves, ncols)).astype(np.int8)
        rows[rng.random((nleaves, ncols)) < 0.04] = -1
        if ncols >= 15:
            rows[:, 3] = -1
            rows[0, 5] = -2
            rows[:, 6] = -2
            rows[nleaves - 1, 6] = 0
        w = G.weights_of(ncat)
    cand = candidates(nleaves, parent)
    if which == "root":
        cand = cand[[int(parent[int(v)]) == len(parent) - 1 for v in cand[:, 0]]]
    elif which == "one":
        cand = cand[:1]
    elif which == "shuffled":
        rng = np.random.default_rng(99 + dim + ncols)
        cand = np.concatenate([cand[rng.permutation(len(cand))], cand[:3]])
    else:
        assert which == "all"
    case = dict(dim=dim, nleaves=nleaves, parent=parent, rows=rows, pi=pi, w=w, P=P, tree=tree, ncat=ncat, cand=cand,
                want=evaluate(dim, nleaves, parent, rows, pi, w, P, cand))
    _cases[key] = case
    return case


# ---- newick helpers of the driver tests -----------------------------------------------------------------------------------------------
def newick_of(names, parent, lengths):
    """A numbered tree (treelik_ref.from_newick's triple) as a newick line, children in ascending node order."""
    kids = children_of(parent)

    def text(v):
        own = names[v] if v < len(names) else "(" + ",".join(text(c) for c in kids[v]) + ")"
        return own if v == len(parent) - 1 else "%s:%.10g" % (own, lengths[v])

    return text(len(parent) - 1) + ";"


def neighbours(names, parent, lengths):
    """Every rooted NNI neighbour of a numbered tree as a newick line: candidate (v, a, c) with a and c exchanged, lengths kept."""
    out = []
    for v, a, c in candidates(len(names), parent):
        p = np.array(parent, np.uint32)
        p[a], p[c] = parent[c], parent[a]
        out.append(newick_of(names, p, lengths))
    return out


def bipartitions(text):
    """The non-trivial bipartitions of a newick line as a set of frozensets (the side without the first name in sorted order)."""
    import transfer_ref as T
    root = T.parse(text.strip())
    everyone = frozenset(T.leaves(root))
    first = min(everyone)
    out = set()

    def walk(node):
        if isinstance(node, str):
            return frozenset([node])
        below = frozenset().union(*[walk(kid) for kid, _, _ in node])
        side = everyone - below if first in below else below
        if 1 < len(side) < len(everyone) - 1:
            out.add(side)
        return below

    walk(root)
    return out
