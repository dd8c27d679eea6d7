"""The joint ancestral reconstruction and the posterior samples of `pgmsa --ml_tree --ml_ancestral_joint / --ml_ancestral_samples` stated
independently of the C++ and the kernels (include/pgm_hip.h: pgm_tree_ancestral_joint, pgm_tree_ancestral_sample), in numpy
float64, vectorised over the sites (and the samples) only.

site_l, site_k and post are treelik_rates_ref.evaluate's without derivatives.  The max-product pass and the stochastic traceback are
restated here with treelik_ref's pieces: every sum a Python loop ascending from 0.0 with one multiply and one add per term, every
maximum a loop that starts with the term of index 0 and lets a later term in only when strictly greater.  The seeded cases are
treelik_rates_ref's without derivatives (category 0 keeps the column of gaps, the row of gaps and the -2 entries); they serve
tests/test_cpu_mljoint.py and tests/test_gpu_mljoint.py."""
import numpy as np

import treelik_rates_ref as G
import treelik_ref as R
from treelik_ref import _apply, _dot, _rescale, children_of

GOLDEN, MIX1, MIX2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _leaf_partials(dim, nleaves, rows):
    states = np.arange(dim)
    return [((rows[l][:, None] < 0) | (rows[l][:, None] == states[None, :])).astype(np.float64) for l in range(nleaves)]


def _argmax_terms(terms):
    """terms: a list of arrays, index ascending.  (the maximum, the first index that holds it) by the rule of the interface."""
    top, arg = terms[0], np.zeros(terms[0].shape, np.int64)
    for j in range(1, len(terms)):
        better = terms[j] > top
        top = np.where(better, terms[j], top)
        arg = np.where(better, j, arg)
    return top, arg


def max_pass(dim, nleaves, parent, rows, pi, X):
    """One category on every site: X[e][0][i, j].  Returns (joint_l, joint_k, the root's state, ptr[v][s, i] of every inner node below
    the root)."""
    nnodes, ncols = len(parent), rows.shape[1]
    root = nnodes - 1
    kids = children_of(parent)
    U = _leaf_partials(dim, nleaves, rows)
    F, ptr = [None] * nnodes, [None] * nnodes
    k = np.zeros(ncols, np.int32)
    for v in range(nleaves, nnodes):
        prod = None
        for c in kids[v]:
            if c < nleaves:
                m = _apply(X[c][0], U[c])
            else:
                m, ptr[c] = _argmax_terms([X[c][0][:, j][None, :] * F[c][:, j][:, None] for j in range(dim)])
            prod = m if prod is None else prod * m
        F[v], hit = _rescale(prod)
        k += hit
    best, arg = _argmax_terms([pi[j] * F[root][:, j] for j in range(dim)])
    return best, k, arg, ptr


def evaluate(dim, nleaves, parent, rows, pi, w, P):
    """pgm_tree_ancestral_joint.  Returns a dict: site_l, site_k, post (ncat x ncols), cat (ncols uint8), joint_state (ninner x ncols
    int8), joint_l, joint_k."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    ncat, nnodes, ncols = len(w), len(parent), rows.shape[1]
    nedges, root = nnodes - 1, nnodes - 1
    X = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    _, cat = _argmax_terms([out["post"][c] for c in range(ncat)])
    passes = [max_pass(dim, nleaves, parent, rows, pi, R.unpack(X[c], nedges, 1, dim)) if np.any(cat == c) else None for c in range(ncat)]
    sites = np.arange(ncols)
    joint_l, joint_k = np.zeros(ncols), np.zeros(ncols, np.int32)
    state = np.full((nnodes - nleaves, ncols), -1, np.int64)
    for c in range(ncat):
        if passes[c] is None:
            continue
        best, k, arg, ptr = passes[c]
        here = cat == c
        joint_l[here], joint_k[here] = best[here], k[here]
        st = np.full((nnodes, ncols), -1, np.int64)
        st[root] = np.where(best == 0.0, -1, arg)
        for v in range(root - 1, nleaves - 1, -1):
            up = st[int(parent[v])]
            st[v] = np.where(up < 0, -1, ptr[v][sites, np.maximum(up, 0)])
        state[:, here] = st[nleaves:, here]
    out.update(cat=cat.astype(np.uint8), joint_state=state.astype(np.int8), joint_l=joint_l, joint_k=joint_k)
    return out


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def uniforms(seed, counter):
    """u of the draws numbered `counter` (a uint64 array): splitmix64 of the state seed + golden * counter, (z >> 11) * 2^-53."""
    counter = np.asarray(counter, np.uint64)
    z = np.full(counter.shape, seed, np.uint64) + GOLDEN * counter
    z = z + GOLDEN
    z = (z ^ (z >> np.uint64(30))) * MIX1
    z = (z ^ (z >> np.uint64(27))) * MIX2
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def pick(q, u):
    """The pick rule on the weights q[..., j] with the uniforms u[...]."""
    m = q.shape[-1]
    T = np.zeros(u.shape)
    for j in range(m):
        T = T + q[..., j]
    target = u * T
    c = np.zeros(u.shape)
    res, last = np.full(u.shape, -2, np.int64), np.full(u.shape, -1, np.int64)
    for j in range(m):
        c = c + q[..., j]
        res = np.where((c > target) & (res == -2), j, res)
        last = np.where(q[..., j] > 0.0, j, last)
    res = np.where(res == -2, last, res)
    return np.where(T == 0.0, -1, res)


def up_pass(dim, nleaves, parent, rows, pi, X):
    """One category: the stored (scaled) partials U[v][s, i] of the inner nodes, and (L, k)."""
    nnodes, ncols = len(parent), rows.shape[1]
    kids = children_of(parent)
    U = _leaf_partials(dim, nleaves, rows) + [None] * (nnodes - nleaves)
    k = np.zeros(ncols, np.int32)
    for v in range(nleaves, nnodes):
        prod = None
        for c in kids[v]:
            S = _apply(X[c][0], U[c])
            prod = S if prod is None else prod * S
        U[v], hit = _rescale(prod)
        k += hit
    return U, _dot(np.broadcast_to(pi, (ncols, dim)), U[nnodes - 1]), k


def sample(dim, nleaves, parent, rows, pi, w, P, nsamp, seed, first_sample=0):
    """pgm_tree_ancestral_sample.  Returns a dict: site_l, site_k, post, samp_cat (ncols x nsamp uint8), samp_state (ninner x ncols x
    nsamp int8)."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    ncat, nnodes, ncols = len(w), len(parent), rows.shape[1]
    nedges, root, ninner = nnodes - 1, nnodes - 1, nnodes - nleaves
    flat = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    X = [R.unpack(flat[c], nedges, 1, dim) for c in range(ncat)]
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    ups = [up_pass(dim, nleaves, parent, rows, pi, X[c]) for c in range(ncat)]
    for c in range(ncat):   # (the same up pass)
        assert R.same_bits(ups[c][1], out["cat_l"][c]) and np.array_equal(ups[c][2], out["cat_k"][c])
    N = np.uint64(first_sample) + np.arange(nsamp, dtype=np.uint64)
    s64 = np.arange(ncols, dtype=np.uint64)
    base = (N[None, :] * np.uint64(ncols) + s64[:, None]) * np.uint64(ninner + 1)   # [s, n]
    sidx = np.broadcast_to(np.arange(ncols)[:, None], (ncols, nsamp))
    cat = pick(np.broadcast_to(out["post"].T[:, None, :], (ncols, nsamp, ncat)), uniforms(seed, base))
    kc = np.maximum(cat, 0)
    state = np.full((nnodes, ncols, nsamp), -1, np.int64)
    Uof = lambda v: np.stack([ups[c][0][v] for c in range(ncat)])[kc, sidx, :]   # [s, n, j]: the partial of the sample's category
    x = pick(pi[None, None, :] * Uof(root), uniforms(seed, base + np.uint64(1 + root - nleaves)))
    state[root] = np.where(cat < 0, -1, x)
    for v in range(root - 1, nleaves - 1, -1):
        up = state[int(parent[v])]
        rows_of_P = np.stack([X[c][v][0] for c in range(ncat)])[kc, np.maximum(up, 0), :]   # [s, n, j] = P_v(up, j) of the sample's category
        x = pick(rows_of_P * Uof(v), uniforms(seed, base + np.uint64(1 + v - nleaves)))
        state[v] = np.where(up < 0, -1, x)
    out.update(samp_cat=np.where(cat < 0, 255, cat).astype(np.uint8), samp_state=state[nleaves:].astype(np.int8))
    return out


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def _finish(key, base, P, w):
    case = dict(dim=base["dim"], nleaves=base["nleaves"], parent=base["parent"], rows=base["rows"], pi=base["pi"], w=w, P=P, tree=base["tree"], ncat=len(w),
                want=evaluate(base["dim"], base["nleaves"], base["parent"], base["rows"], base["pi"], w, P))
    _cases[key] = case
    return case


def make_case(dim, ncols, tree, ncat, weights="equal"):
    """treelik_rates_ref.make_case without derivatives (P alone) and the joint expectation, computed once per process."""
    key = (dim, ncols, tree, ncat, weights)
    if key in _cases:
        return _cases[key]
    base = G.make_case(dim, ncols, tree, ncat, False, weights)
    return _finish(key, base, base["P"], base["w"])


def make_mixed_scaling_case(dim, scale0=1.0, least=1):
    """treelik_rates_ref.make_mixed_scaling_case (the caterpillar of 96 leaves, 17 columns, two categories) with the first matrix of
    every edge alone."""
    key = ("mixed", dim, scale0, least)
    if key in _cases:
        return _cases[key]
    base = G.make_mixed_scaling_case(dim, scale0, least)
    nedges = len(base["parent"]) - 1
    P = np.ascontiguousarray(base["P"].reshape(2, nedges, 3, dim * dim)[:, :, 0]).reshape(-1)
    case = _finish(key, base, P, base["w"])
    assert R.same_bits(case["want"]["post"], base["want"]["post"]) and np.array_equal(case["want"]["site_k"], base["want"]["site_k"])
    return case


def with_want(c):
    c = dict(c)
    c["want"] = evaluate(c["dim"], c["nleaves"], c["parent"], c["rows"], c["pi"], c["w"], c["P"])
    return c


_samples = {}


def samples_of(case, nsamp, seed, first_sample=0, key=None):
    """sample() on a case, computed once per process when the case has a key."""
    k = (key, nsamp, seed, first_sample)
    if key is not None and k in _samples:
        return _samples[k]
    got = sample(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], nsamp, seed, first_sample)
    if key is not None:
        _samples[k] = got
    return got
