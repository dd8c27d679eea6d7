"""The tree likelihood of `pgmsa --ml_tree` stated independently of the C++ and the kernels (include/pgm_hip.h:
pgm_tree_likelihood), in numpy float64, vectorised over the sites only.

Every sum over states is a Python loop over its index ascending that starts from 0.0 and does one multiply and one add per term (two
numpy ufunc calls: nothing is fused), products run over the children in node order, the scaling rule and the chunk-of-16 summation
are the interface's: the bits of evaluate() are the contract's.  The helpers around it (trees, models, rows of a FASTA) serve
tests/test_cpu_mltree.py and tests/test_gpu_mltree.py."""
import math
import os

import numpy as np

import mldist_general_ref as M
import transfer_ref as T

CHUNK = 16
TINY, SCALE = 2.0 ** -256, 2.0 ** 256
ROOT = 0xFFFFFFFF
T_MIN, T_MAX = 1e-6, 10.0


# ---- the statement ------------------------------------------------------------------------------------------------------------
def children_of(parent):
    kids = [[] for _ in parent]
    for v, p in enumerate(parent):
        if int(p) != ROOT:
            kids[int(p)].append(v)
    return kids


def _apply(X, u):
    """out[s, i] = sum over j ascending of X[i, j] * u[s, j]."""
    acc = np.zeros_like(u)
    for j in range(X.shape[0]):
        acc = acc + X[:, j][None, :] * u[:, j][:, None]
    return acc


def _rescale(v):
    m = v.max(axis=1)
    hit = (m < TINY) & (m > 0.0)
    return np.where(hit[:, None], v * SCALE, v), hit


def _dot(a, b):
    """out[s] = sum over i ascending of a[s, i] * b[s, i]."""
    acc = np.zeros(a.shape[0])
    for i in range(a.shape[1]):
        acc = acc + a[:, i] * b[:, i]
    return acc


def unpack(P, nedges, nx, dim):
    """The C ABI's matrices as X[e][x][i, j]."""
    return np.asarray(P, np.float64).reshape(nedges, nx, dim, dim).transpose(0, 1, 3, 2)


def pack(X):
    """X[e][x][i, j] -> the C ABI's layout (every matrix column-major)."""
    return np.ascontiguousarray(np.asarray(X, np.float64).transpose(0, 1, 3, 2)).reshape(-1)


def evaluate(dim, nleaves, parent, rows, pi, P, derivs=True):
    """pgm_tree_likelihood.  parent: nnodes (the root's ROOT); rows: nleaves x ncols int8; P: the C ABI's flat array.
    Returns a dict: site_l, site_k, and with derivs d1, d2 and the per-site ratios g, h (nedges x ncols)."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    nnodes, ncols = len(parent), rows.shape[1]
    nedges, root = nnodes - 1, nnodes - 1
    X = unpack(P, nedges, 3 if derivs else 1, dim)
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
    out = dict(site_l=_dot(np.broadcast_to(pi, (ncols, dim)), U[root]), site_k=k)
    if not derivs:
        return out
    O = [None] * nnodes
    g, h = np.zeros((nedges, ncols)), np.zeros((nedges, ncols))
    for v in range(root, nleaves - 1, -1):
        if v == root:
            base = np.broadcast_to(pi, (ncols, dim)).copy()
        else:
            base = np.zeros((ncols, dim))
            for hh in range(dim):
                base = base + O[v][:, hh][:, None] * X[v][0][hh, :][None, :]
        S = {c: _apply(X[c][0], U[c]) for c in kids[v]}
        for c in kids[v]:
            o = base
            for sib in kids[v]:
                if sib != c:
                    o = o * S[sib]
            o, _ = _rescale(o)
            O[c] = o
            A0 = _dot(o, S[c])
            A1 = _dot(o, _apply(X[c][1], U[c]))
            A2 = _dot(o, _apply(X[c][2], U[c]))
            with np.errstate(all="ignore"):
                g[c] = A1 / A0
                h[c] = A2 / A0 - g[c] * g[c]
    out.update(g=g, h=h, d1=chunk_sums(g), d2=chunk_sums(h))
    return out


def chunk_sums(G):
    """Per row: the sites ascending within consecutive chunks of 16, then the chunk sums ascending."""
    total = np.zeros(G.shape[0])
    for s0 in range(0, G.shape[1], CHUNK):
        acc = np.zeros(G.shape[0])
        for s in range(s0, min(G.shape[1], s0 + CHUNK)):
            acc = acc + G[:, s]
        total = total + acc
    return total


def site_lnl(site_l, site_k):
    return np.log(site_l) - site_k.astype(np.float64) * (256.0 * math.log(2.0))


def lnl_of(site_l, site_k):
    total = 0.0
    for v in site_lnl(site_l, site_k):
        total = total + float(v)
    return total


# ---- trees --------------------------------------------------------------------------------------------------------------------
def balanced(n):
    """A rooted binary tree of n leaves, as even as it gets; parent array (leaves 0 .. n-1, children before parents, root last)."""
    parent = [ROOT] * n

    def build(lo, hi):
        if hi - lo == 1:
            return lo
        mid = (lo + hi) // 2
        a, b = build(lo, mid), build(mid, hi)
        parent.append(ROOT)
        v = len(parent) - 1
        parent[a] = parent[b] = v
        return v

    build(0, n)
    return np.array(parent, np.uint32)


def caterpillar(n):
    """((((0,1),2),3) ...): n - 1 levels."""
    parent = [ROOT] * n
    below = 0
    for l in range(1, n):
        parent.append(ROOT)
        v = len(parent) - 1
        parent[below] = parent[l] = v
        below = v
    return np.array(parent, np.uint32)


def trifurcating(n):
    """Three balanced subtrees under one root; n >= 3."""
    parent = [ROOT] * n
    cuts = [0, n // 3, 2 * n // 3, n]
    tops = []
    for a, b in zip(cuts, cuts[1:]):
        sub = balanced(b - a)
        base = len(parent)
        ids = [a + v if v < b - a else base + (v - (b - a)) for v in range(len(sub))]
        parent.extend([ROOT] * (len(sub) - (b - a)))
        for v, p in enumerate(sub):
            if int(p) != ROOT:
                parent[ids[v]] = ids[int(p)]
        tops.append(ids[len(sub) - 1])
    parent.append(ROOT)
    for t in tops:
        parent[t] = len(parent) - 1
    return np.array(parent, np.uint32)


def inner_trifurcation():
    """Six leaves: node 6 = (0, 1, 2), 7 = (6, 3), 8 = (7, 4), the root 9 = (8, 5): a non-root inner node with three children."""
    return 6, np.array([6, 6, 6, 7, 8, 9, 7, 8, 9, ROOT], np.uint32)


def inner_quadrifurcation():
    """Seven leaves: 7 = (0, 1), 8 = (2, 3), 9 = (4, 5, 7, 8), the root 10 = (6, 9): a non-root inner node with four children, two of
    them inner, under a binary root."""
    return 7, np.array([7, 7, 8, 8, 9, 9, 10, 9, 9, 10, ROOT], np.uint32)


def four_leaves_beside_a_cherry():
    """Six leaves: 6 = (0, 1, 2, 3), 7 = (4, 5), the root 8 = (6, 7): a non-root inner node whose four children are all leaves."""
    return 6, np.array([6, 6, 6, 6, 7, 7, 8, 8, ROOT], np.uint32)


def star(n):
    """A root with n leaf children and no other inner node."""
    return n, np.array([n] * n + [ROOT], np.uint32)


def mixed_root():
    """Six leaves: 6 = (0, 1, 2), 7 = (3, 4), the root 8 = (5, 6, 7): a root with a leaf, a trifurcation and a cherry below it."""
    return 6, np.array([6, 6, 6, 7, 7, 8, 8, 8, ROOT], np.uint32)


def from_newick(text):
    """The numbering of ml_tree_topology: the leaves in sorted-name order, the inner nodes in post-order, the root last.
    Returns (names, parent, lengths per edge)."""
    root = T.parse(text.strip())
    names = sorted(T.leaves(root))
    index = {n: k for k, n in enumerate(names)}
    assert len(index) == len(names)
    parent, length = [ROOT] * len(names), [None] * len(names)

    def walk(node):
        if isinstance(node, str):
            return index[node]
        ids = [(walk(kid), float(ln[1:])) for kid, ln, _ in node]
        parent.append(ROOT)
        length.append(None)
        v = len(parent) - 1
        for c, t in ids:
            parent[c], length[c] = v, t
        return v

    walk(root)
    return names, np.array(parent, np.uint32), np.array(length[:-1], np.float64)


def shape_of(text):
    """The topology of a newick line without its numbers: nested sorted tuples of leaf names."""
    def walk(node):
        return node if isinstance(node, str) else tuple(sorted((walk(kid) for kid, _, _ in node), key=repr))
    return walk(T.parse(text.strip()))


# ---- models -------------------------------------------------------------------------------------------------------------------
def shipped(name):
    """(Q, pi) of host/data/<name> as ModelFactory's constructor sets them up."""
    Q = M.read_qmat(os.path.join(M.DATA, name))
    n = Q.shape[0]
    A = Q.T.copy()
    A[n - 1, :] = 1.0
    b = np.zeros(n); b[n - 1] = 1.0
    pi = np.linalg.solve(A, b)
    return M.normalised(Q, pi), pi


def custom(path, dim):
    """(Q, pi) of a --custom_model file (ModelFactory::readCustom): the exchangeabilities themselves as the generator."""
    tok = [float(x) for x in open(path).read().split()]
    Q = np.zeros((dim, dim))
    k = 0
    for i in range(1, dim):
        for j in range(i):
            Q[i, j] = Q[j, i] = tok[k]; k += 1
    pi = np.array(tok[k:k + dim])
    pi = pi / pi.sum()
    return M.normalised(Q, pi), pi


def matrices(Q, lengths, derivs=True):
    """The C ABI's P for the edges' lengths: exp(Q t) by scipy, Q P and Q Q P by numpy."""
    from scipy.linalg import expm
    X = []
    for t in lengths:
        P = expm(Q * float(t))
        X.append([P, Q @ P, Q @ (Q @ P)] if derivs else [P])
    return pack(np.array(X))


# ---- the rows of a written alignment ----------------------------------------------------------------------------------------------
_AA = "ACDEFGHIKLMNPQRSTVWY"
_NT = {"T": 0, "U": 0, "C": 1, "A": 2, "G": 3}


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:]
            seqs[name] = ""
        elif name is not None:
            seqs[name] += line
    return seqs


def rows_of(seqs, names, kind):
    """State values of the written rows: 0 .. dim-1, -1 a gap, -2 a residue without a value.  kind: "aa", "dna" or "codon"."""
    out = []
    for n in names:
        s = seqs[n].upper()
        if kind == "aa":
            r = [-1 if c == "-" else _AA.find(c) if c in _AA else -2 for c in s]
        elif kind == "dna":
            r = [-1 if c == "-" else _NT.get(c, -2) for c in s]
        else:
            r = []
            for p in range(0, len(s) - 2, 3):
                cod = s[p:p + 3]
                if any(c in "-_. " for c in cod):
                    r.append(-1)
                elif all(c in _NT for c in cod):
                    c = 16 * _NT[cod[0]] + 4 * _NT[cod[1]] + _NT[cod[2]]
                    r.append(-2 if c in (10, 11, 14) else c - (c > 10) - (c > 11) - (c > 14))
                else:
                    r.append(-2)
        out.append(r)
    assert len({len(r) for r in out}) == 1
    return np.array(out, np.int8)


# ---- seeded cases of the kernel test and of its host companion ------------------------------------------------------------------------
TREES = {
    "two": lambda: (2, balanced(2)),
    "three": lambda: (3, caterpillar(3)),
    "balanced8": lambda: (8, balanced(8)),
    "balanced24": lambda: (24, balanced(24)),
    "trifurcating": lambda: (7, trifurcating(7)),
    "caterpillar96": lambda: (96, caterpillar(96)),
    # polytomies below the root, and roots of other arities (tests/test_cpu_treelik_shapes.py)
    "inner3": inner_trifurcation,
    "inner4": inner_quadrifurcation,
    "leaves4": four_leaves_beside_a_cherry,
    "star5": lambda: star(5),
    "mixed3": mixed_root,
    "balanced32770": lambda: (32770, balanced(32770)),   # 65538 edges: more than the second grid dimension holds
}
_cases = {}


def make_case(dim, ncols, tree, derivs=True, want=True):
    """One seeded case and its expectation (computed once per process): a dict with nleaves, parent, rows, pi, P and `want`
    (None when not asked for: the inputs alone, for a caller with an expectation of its own).
    P: row-stochastic matrices of entries above 0.01 / dim, P' and P'' signed; for the caterpillar every entry of all three in
    [0.03, 0.07].  Columns from 15 sites on: site 3 is all gaps, sites 5 and 6 hold -2 entries; from 3 leaves on leaf 1 is all gaps
    in half of the trees' cases (by dim); 4 % of the other entries are gaps.  The caterpillar keeps its even sites free of gaps."""
    key = (dim, ncols, tree, derivs)
    if key in _cases and (_cases[key]["want"] is not None or not want):
        return _cases[key]
    nleaves, parent = TREES[tree]()
    nedges = len(parent) - 1
    rng = np.random.default_rng(1000 * dim + 7 * ncols + sum(map(ord, tree)))
    pi = rng.dirichlet(np.ones(dim) * 4)
    if tree == "caterpillar96":
        X = rng.uniform(0.03, 0.07, (nedges, 3, dim, dim))
    else:
        P0 = rng.uniform(0.01, 1.0, (nedges, dim, dim))
        P0 /= P0.sum(axis=2, keepdims=True)
        X = np.stack([P0, rng.normal(0, 0.5, (nedges, dim, dim)), rng.normal(0, 1.0, (nedges, dim, dim))], axis=1)
    if not derivs:
        X = X[:, :1]
    rows = rng.integers(0, dim, (nleaves, ncols)).astype(np.int8)
    gaps = rng.random((nleaves, ncols)) < 0.04
    if tree == "caterpillar96":
        gaps[:, 0::2] = False
    rows[gaps] = -1
    if ncols >= 15:
        rows[:, 3] = -1
        rows[0, 5] = -2
        rows[:, 6] = -2
        rows[nleaves - 1, 6] = 0
    if nleaves >= 3 and dim in (4, 61) and tree != "caterpillar96":
        rows[1, :] = -1
    P = pack(X)
    case = dict(dim=dim, nleaves=nleaves, parent=parent, rows=rows, pi=pi, P=P, derivs=derivs, tree=tree,
                want=evaluate(dim, nleaves, parent, rows, pi, P, derivs) if want else None)
    _cases[key] = case
    return case


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
