"""The tree likelihood under rate categories of `pgmsa --ml_tree --ml_gamma` stated independently of the C++ and the kernels (DESIGN
3.18; include/pgm_hip.h: pgm_tree_likelihood_rates), in numpy float64, vectorised over the sites only.

The walk of one category is restated here with treelik_ref's pieces (it must return q_c = A''/A, which treelik_ref.evaluate folds
into h); the categories are then combined in the order of the interface, every sum a Python loop ascending from 0.0 with one
multiply and one add per term.  gamma_rates is the discrete gamma by scipy.  The seeded cases serve tests/test_cpu_mlgamma.py and
tests/test_gpu_mlgamma.py."""
import numpy as np

import treelik_ref as R
from treelik_ref import _apply, _dot, _rescale, children_of


def walk(dim, nleaves, parent, rows, pi, X, derivs):
    """One category: X[e][x][i, j].  Returns (L, k) and with derivs the per-site ratios g_c = A'/A, q_c = A''/A (nedges x ncols)."""
    nnodes, ncols = len(parent), rows.shape[1]
    nedges, root = nnodes - 1, nnodes - 1
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
    if not derivs:
        return L, k, None, None
    O = [None] * nnodes
    g, q = np.zeros((nedges, ncols)), np.zeros((nedges, ncols))
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
                q[c] = A2 / A0
    return L, k, g, q


def evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=True):
    """pgm_tree_likelihood_rates.  w: ncat weights; P: the C ABI's flat array, category-major.  Returns a dict: site_l, site_k, post
    (ncat x ncols), the categories' (L, k), and with derivs d1, d2 and the per-site g, h (nedges x ncols)."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    ncat, nedges, ncols, nx = len(w), len(parent) - 1, rows.shape[1], 3 if derivs else 1
    X = np.asarray(P, np.float64).reshape(ncat, nedges * nx * dim * dim)
    cats = [walk(dim, nleaves, parent, rows, pi, R.unpack(X[c], nedges, nx, dim), derivs) for c in range(ncat)]
    kc = np.array([c[1] for c in cats], np.int32)
    site_k = kc.min(axis=0)
    terms, site_l = [], np.zeros(ncols)
    for c in range(ncat):
        term = w[c] * cats[c][0]
        for n in range(int((kc[c] - site_k).max())):
            term = np.where(kc[c] - site_k > n, term * R.TINY, term)
        terms.append(term)
        site_l = site_l + term
    with np.errstate(all="ignore"):
        post = np.array([term / site_l for term in terms])
    out = dict(site_l=site_l, site_k=site_k.astype(np.int32), post=post, cat_l=np.array([c[0] for c in cats]), cat_k=kc)
    if not derivs:
        return out
    g, q = np.zeros((nedges, ncols)), np.zeros((nedges, ncols))
    for c in range(ncat):
        g = g + post[c][None, :] * cats[c][2]
        q = q + post[c][None, :] * cats[c][3]
    h = q - g * g
    out.update(g=g, h=h, d1=R.chunk_sums(g), d2=R.chunk_sums(h), cat_g=np.array([c[2] for c in cats]))
    return out


# ---- the discrete gamma ---------------------------------------------------------------------------------------------------------------
def gamma_rates(alpha, K):
    """K equally probable categories of Gamma(shape alpha, scale 1 / alpha), each rate the mean of its category (Yang 1994), then
    divided by their average."""
    from scipy.special import gammainc
    from scipy.stats import gamma
    cuts = np.concatenate([[0.0], gamma.ppf(np.arange(1, K) / K, a=alpha, scale=1.0 / alpha), [np.inf]])
    upper = gammainc(alpha + 1.0, alpha * cuts)
    r = K * (upper[1:] - upper[:-1])
    return r / (r.sum() / K)


def matrices(Q, lengths, rates, derivs=True):
    """The C ABI's P for the edges' lengths and the categories' rates: P(r t), r Q P, r^2 Q Q P."""
    from scipy.linalg import expm
    out = []
    for r in rates:
        X = []
        for t in lengths:
            P = expm(Q * float(r) * float(t))
            X.append([P, r * (Q @ P), r * r * (Q @ (Q @ P))] if derivs else [P])
        out.append(R.pack(np.array(X)))
    return np.concatenate(out)


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def weights_of(ncat, kind="equal"):
    if kind == "equal":
        return np.full(ncat, 1.0 / ncat) if ncat > 1 else np.array([1.0])
    assert kind == "unequal" and ncat == 4
    return np.array([0.1, 0.2, 0.3, 0.4])


def make_case(dim, ncols, tree, ncat, derivs=True, weights="equal", plain_want=True):
    """Category 0 is treelik_ref.make_case's case itself (rows, pi, its matrices); the further categories have matrices of their own,
    drawn the same way.  With ncat == 1 the inputs are exactly those of treelik_ref.make_case.  plain_want=False: that case's own
    expectation is not computed (a large tree)."""
    key = (dim, ncols, tree, ncat, derivs, weights)
    if key in _cases:
        return _cases[key]
    base = R.make_case(dim, ncols, tree, derivs, want=plain_want)
    nedges = len(base["parent"]) - 1
    rng = np.random.default_rng(77 + 1000 * dim + 7 * ncols + 13 * ncat + sum(map(ord, tree)))
    parts = [base["P"]]
    for c in range(1, ncat):
        if tree == "caterpillar96":
            X = rng.uniform(0.03, 0.07, (nedges, 3, dim, dim))
        else:
            P0 = rng.uniform(0.01, 1.0, (nedges, dim, dim))
            P0 /= P0.sum(axis=2, keepdims=True)
            X = np.stack([P0, rng.normal(0, 0.5, (nedges, dim, dim)), rng.normal(0, 1.0, (nedges, dim, dim))], axis=1)
        parts.append(R.pack(X if derivs else X[:, :1]))
    P = np.concatenate(parts)
    w = weights_of(ncat, weights)
    case = dict(dim=dim, nleaves=base["nleaves"], parent=base["parent"], rows=base["rows"], pi=base["pi"], w=w, P=P, derivs=derivs, tree=tree, ncat=ncat,
                want=evaluate(dim, base["nleaves"], base["parent"], base["rows"], base["pi"], w, P, derivs))
    _cases[key] = case
    return case


def make_mixed_scaling_case(dim, scale0=1.0, least=1):
    """The caterpillar of 96 leaves, 17 columns, two categories: category 0 has treelik_ref's caterpillar matrices (every entry in
    [0.03, 0.07]) times scale0, so it rescales; category 1 has row-stochastic matrices and rescales later or never.  Asserts that some column without
    gaps has k_0 - k_1 >= least: the shift by 2^-256 ran there `least` times or more.  From 5 shifts on the term is an exact 0.0
    (w L <= 1 and 2^-1280 is below the smallest double), asserted as well."""
    key = ("mixed", dim, scale0, least)
    if key in _cases:
        return _cases[key]
    base = R.make_case(dim, 17, "caterpillar96")
    nedges = len(base["parent"]) - 1
    rng = np.random.default_rng(4242 + dim)
    P0 = rng.uniform(0.01, 1.0, (nedges, dim, dim))
    P0 /= P0.sum(axis=2, keepdims=True)
    X = np.stack([P0, rng.normal(0, 0.5, (nedges, dim, dim)), rng.normal(0, 1.0, (nedges, dim, dim))], axis=1)
    P = np.concatenate([base["P"] * scale0, R.pack(X)])
    w = weights_of(2)
    want = evaluate(dim, base["nleaves"], base["parent"], base["rows"], base["pi"], w, P, True)
    full = (base["rows"] >= 0).all(axis=0)
    diff = want["cat_k"][0] - want["cat_k"][1]
    assert np.any(diff[full] >= least), (diff, least)
    if least >= 5:
        hit = full & (diff >= 5)
        assert np.all(want["post"][0][hit] == 0.0) and np.all(want["post"][1][hit] == 1.0)
    else:
        assert np.any((want["post"][0][full] > 0.0) & (want["post"][0][full] < 1e-60))   # tiny, but the statement's
    case = dict(dim=dim, nleaves=base["nleaves"], parent=base["parent"], rows=base["rows"], pi=base["pi"], w=w, P=P, derivs=True, tree="caterpillar96", ncat=2,
                want=want, full=full, diff=diff)
    _cases[key] = case
    return case
