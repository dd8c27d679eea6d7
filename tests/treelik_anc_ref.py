"""The marginal ancestral states of `pgmsa --ml_tree --ml_ancestral` stated independently of the C++ and the kernels (DESIGN 3.19;
include/pgm_hip.h: pgm_tree_ancestral), in numpy float64, vectorised over the sites only.

site_l, site_k and post are treelik_rates_ref.evaluate's without derivatives; the walk of one category is restated here with
treelik_ref's pieces (it must keep the partials and run the down pass with P alone), every sum a Python loop ascending from 0.0 with
one multiply and one add per term.  The seeded cases are treelik_rates_ref's without derivatives; they serve
tests/test_cpu_mlancestral.py and tests/test_gpu_mlancestral.py."""
import numpy as np

import treelik_rates_ref as G
import treelik_ref as R
from treelik_ref import _apply, _dot, _rescale, children_of


def walk(dim, nleaves, parent, rows, pi, X):
    """One category: X[e][0][i, j], P alone.  Returns (L, k) of the up pass and a[v - nleaves][s, i] = B_v(i) U_v(i) / Z."""
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
    a = np.zeros((nnodes - nleaves, ncols, dim))
    for v in range(root, nleaves - 1, -1):
        if v == root:
            base = np.broadcast_to(pi, (ncols, dim)).copy()
        else:
            base = np.zeros((ncols, dim))
            for hh in range(dim):
                base = base + O[v][:, hh][:, None] * X[v][0][hh, :][None, :]
        m = base * U[v]
        Z = np.zeros(ncols)
        for i in range(dim):
            Z = Z + m[:, i]
        with np.errstate(all="ignore"):
            a[v - nleaves] = np.where((Z == 0.0)[:, None], 0.0, m / Z[:, None])
        S = {c: _apply(X[c][0], U[c]) for c in kids[v]}
        for c in kids[v]:
            if c < nleaves:
                continue
            o = base
            for sib in kids[v]:
                if sib != c:
                    o = o * S[sib]
            O[c], _ = _rescale(o)
    return L, k, a


def evaluate(dim, nleaves, parent, rows, pi, w, P):
    """pgm_tree_ancestral.  w: ncat weights; P: the C ABI's flat array (P alone), category-major.  Returns a dict: site_l, site_k, post
    (ncat x ncols), anc_post (ninner x ncols x dim), anc_state (ninner x ncols int8), anc_prob (ninner x ncols), cat_a (the
    categories' posteriors)."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    ncat, nedges, ncols = len(w), len(parent) - 1, rows.shape[1]
    X = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    cats = [walk(dim, nleaves, parent, rows, pi, R.unpack(X[c], nedges, 1, dim)) for c in range(ncat)]
    for c in range(ncat):   # (the same up pass)
        assert R.same_bits(cats[c][0], out["cat_l"][c]) and np.array_equal(cats[c][1], out["cat_k"][c])
    post = out["post"]
    anc = np.zeros((len(parent) - nleaves, ncols, dim))
    for c in range(ncat):
        anc = anc + post[c][None, :, None] * cats[c][2]
    state = np.full(anc.shape[:2], -1, np.int8)
    top = np.zeros(anc.shape[:2])
    for i in range(dim):
        better = anc[:, :, i] > top
        state = np.where(better, np.int8(i), state)
        top = np.where(better, anc[:, :, i], top)
    out.update(anc_post=anc, anc_state=state.astype(np.int8), anc_prob=top, cat_a=np.array([c[2] for c in cats]))
    return out


def presence(nleaves, parent, rows):
    """The gap rule of --ml_ancestral: present[v - nleaves][s] iff at least two of the directions at v (its children, and its parent's
    side unless v is the root) hold a leaf whose row is not -1."""
    parent = np.asarray(parent, np.uint32)
    nnodes, ncols = len(parent), rows.shape[1]
    root = nnodes - 1
    kids = children_of(parent)
    r = np.zeros((nnodes, ncols), np.int64)
    r[:nleaves] = np.asarray(rows) != -1
    for v in range(nleaves, nnodes):
        r[v] = sum(r[c] for c in kids[v])
    out = np.zeros((nnodes - nleaves, ncols), bool)
    for v in range(nleaves, nnodes):
        count = sum((r[c] > 0).astype(np.int64) for c in kids[v])
        if v != root:
            count = count + (r[root] - r[v] > 0)
        out[v - nleaves] = count >= 2
    return out


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def _finish(key, base, P, w):
    case = dict(dim=base["dim"], nleaves=base["nleaves"], parent=base["parent"], rows=base["rows"], pi=base["pi"], w=w, P=P, tree=base["tree"], ncat=len(w),
                want=evaluate(base["dim"], base["nleaves"], base["parent"], base["rows"], base["pi"], w, P))
    _cases[key] = case
    return case


def make_case(dim, ncols, tree, ncat, weights="equal"):
    """treelik_rates_ref.make_case without derivatives (P alone) and its expectation, computed once per process."""
    key = (dim, ncols, tree, ncat, weights)
    if key in _cases:
        return _cases[key]
    base = G.make_case(dim, ncols, tree, ncat, False, weights)
    return _finish(key, base, base["P"], base["w"])


def make_mixed_scaling_case(dim, scale0=1.0, least=1):
    """treelik_rates_ref.make_mixed_scaling_case with the first matrix of every edge alone: the two categories rescale a different
    number of times, and from 5 shifts on category 0's share of the mixture is an exact 0.0."""
    key = ("mixed", dim, scale0, least)
    if key in _cases:
        return _cases[key]
    base = G.make_mixed_scaling_case(dim, scale0, least)
    nedges = len(base["parent"]) - 1
    P = np.ascontiguousarray(base["P"].reshape(2, nedges, 3, dim * dim)[:, :, 0]).reshape(-1)
    case = _finish(key, base, P, base["w"])
    assert R.same_bits(case["want"]["post"], base["want"]["post"]) and np.array_equal(case["want"]["site_k"], base["want"]["site_k"])
    case.update(full=base["full"], diff=base["diff"])
    return case
