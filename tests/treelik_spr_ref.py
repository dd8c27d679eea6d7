"""The subtree pruning and regrafting scores of `pgmsa --ml_tree --ml_search --ml_spr` stated independently of the C++ and the kernel
(include/pgm_hip.h: pgm_tree_spr), in numpy float64, vectorised over the sites only.

site_l, site_k and post are treelik_rates_ref.evaluate's without derivatives; the partials U and the outside vectors O of a category are
treelik_nni_ref.walk's; every sum is a Python loop ascending from 0.0 with one multiply and one add per term (treelik_ref's _apply and
_dot, and _down below).  Beside the statement: the path of a candidate, the lister of every valid candidate within a radius, the
regrafted tree itself (renumbered, with the matrices of its edges) for a brute-force evaluation, and the seeded cases of
tests/test_cpu_mlspr.py and tests/test_gpu_mlspr.py."""
import numpy as np

import treelik_anc_ref as A
import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
from treelik_ref import _apply, _dot, _rescale, children_of

ROOT = R.ROOT
MAXPATH = 16


# ---- candidates ------------------------------------------------------------------------------------------------------------------------
def _ancestors(parent, x):
    out = [int(x)]
    while int(parent[out[-1]]) != ROOT:
        out.append(int(parent[out[-1]]))
    return out


def path_of(parent, v, y, kids=None):
    """(up, down) of a valid candidate: up = [a_0 = p, .., a_J = a], down = [c_1, .., c_M = y]; None for a candidate the entry refuses
    (the length of the path aside).  kids: children_of(parent), where the caller has it."""
    n = len(parent)
    if not (0 <= v < n and 0 <= y < n) or int(parent[v]) == ROOT or int(parent[y]) == ROOT:
        return None
    p = int(parent[v])
    above_y = _ancestors(parent, y)
    if v in above_y:
        return None
    arity = len(kids[p]) if kids is not None else sum(1 for x in parent if int(x) == p)
    if arity == 2 and (int(parent[p]) == ROOT or y == p or int(parent[y]) == p):
        return None
    up = []
    for x in _ancestors(parent, p):
        up.append(x)
        if x in above_y:
            break
    down = above_y[:above_y.index(up[-1])][::-1]
    return up, down


def candidates(nleaves, parent, radius=MAXPATH):
    """Every valid candidate whose path has at most `radius` edges: v ascending, then y ascending.  The path has as many edges as the
    tree has between p and y, so the targets are the nodes within `radius` steps of p that are not reached through v; every one of
    them goes through path_of (candidates_by_path: the same list by trying every pair)."""
    kids = children_of(parent)
    out = []
    for v in range(len(parent) - 1):
        p = int(parent[v])
        near, edge = {p: 0}, [p]
        for step in range(1, radius + 1):
            nxt = []
            for x in edge:
                for z in kids[x] + ([int(parent[x])] if int(parent[x]) != ROOT else []):
                    if z != v and z not in near:
                        near[z] = step
                        nxt.append(z)
            edge = nxt
        for y in sorted(near):
            path = path_of(parent, v, y, kids)
            if path is not None:
                assert len(path[0]) - 1 + len(path[1]) == near[y]
                out.append((v, y))
    return np.array(out, np.uint32).reshape(-1, 2)


def candidates_by_path(nleaves, parent, radius=MAXPATH):
    out = []
    for v in range(len(parent) - 1):
        for y in range(len(parent) - 1):
            path = path_of(parent, v, y)
            if path is not None and len(path[0]) - 1 + len(path[1]) <= radius:
                out.append((v, y))
    return np.array(out, np.uint32).reshape(-1, 2)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def _down(g, X):
    """out[s, i] = sum over h ascending of g[s, h] * X[h, i]."""
    acc = np.zeros_like(g)
    for h in range(X.shape[0]):
        acc = acc + g[:, h][:, None] * X[h, :][None, :]
    return acc


def evaluate(dim, nleaves, parent, rows, pi, w, P, Ph, cand):
    """pgm_tree_spr.  cand: rows (v, y).  Returns a dict: site_l, site_k, post (ncat x ncols), rho (ncand x ncols), and per category
    the ratios cat_rho and the counts cat_km, cat_kp of the two chains (ncat x ncand x ncols each)."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    cand = np.asarray(cand, np.int64).reshape(-1, 2)
    ncat, nedges, ncols, ncand = len(w), len(parent) - 1, rows.shape[1], len(cand)
    root = len(parent) - 1
    kids = children_of(parent)
    Xall = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    Hall = np.asarray(Ph, np.float64).reshape(ncat, nedges * dim * dim)
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    post = out["post"]
    walks = []
    for k in range(ncat):
        X = R.unpack(Xall[k], nedges, 1, dim)
        _, _, U, O = N.walk(dim, nleaves, parent, rows, pi, X)
        S_all = [_apply(X[x][0], U[x]) if x != root else None for x in range(len(parent))]   # S_x of every node below the root, once
        walks.append((X, R.unpack(Hall[k], nedges, 1, dim), U, O, S_all))
    rho = np.zeros((ncand, ncols))
    cat_rho = np.zeros((ncat, ncand, ncols))
    cat_km, cat_kp = np.zeros((ncat, ncand, ncols), np.int32), np.zeros((ncat, ncand, ncols), np.int32)
    for q, (v, y) in enumerate(cand):
        v, y = int(v), int(y)
        path = path_of(parent, v, y)
        assert path is not None, (v, y)
        up, down = path
        J, M = len(up) - 1, len(down)
        assert J + M <= MAXPATH
        p = up[0]
        mixed = np.zeros(ncols)
        for k in range(ncat):
            X, H, U, O, S_all = walks[k]
            S = lambda x: S_all[x]
            count = [np.zeros(ncols, np.int32), np.zeros(ncols, np.int32)]

            def rule(vec, sign):
                vec, hit = _rescale(vec)
                count[sign] = count[sign] + hit.astype(np.int32)
                return vec

            Sv = S(v)
            E = [None, None]
            if J >= 1 or M == 0:
                first = None
                for c in kids[p]:
                    if c != v:
                        first = S(c) if first is None else first * S(c)
                E = [rule(first, 0), rule(first * Sv, 1)]
            Mup = [None, None]
            for j in range(1, J + 1):
                Mup = [_apply(X[up[j - 1]][0], E[0]), _apply(X[up[j - 1]][0], E[1])]
                if j < J or M == 0:
                    nxt = list(Mup)
                    for c in kids[up[j]]:
                        if c != up[j - 1]:
                            Sc = S(c)
                            nxt = [nxt[0] * Sc, nxt[1] * Sc]
                    E = [rule(nxt[0], 0), rule(nxt[1], 1)]
            if M == 0:
                Xv = rule(Sv * _apply(H[y][0], E[0]), 0)
                W = _apply(H[y][0], Xv)
                Nn = _dot(O[y], W)
                Dd = _dot(O[y], _apply(X[y][0], E[1]))
            else:
                a = up[J]
                B = N._base(dim, ncols, pi, X, O, a, root)
                if J >= 1:
                    Gm, Gp = B * Mup[0], B * Mup[1]
                    for c in kids[a]:
                        if c != up[J - 1] and c != down[0]:
                            Sc = S(c)
                            Gm, Gp = Gm * Sc, Gp * Sc
                else:
                    Gm = B
                    for c in kids[a]:
                        if c != v and c != down[0]:
                            Gm = Gm * S(c)
                    Gp = Gm * Sv
                Gm, Gp = rule(Gm, 0), rule(Gp, 1)
                for m in range(1, M):
                    Gm, Gp = _down(Gm, X[down[m - 1]][0]), _down(Gp, X[down[m - 1]][0])
                    for c in kids[down[m - 1]]:
                        if c != down[m]:
                            Sc = S(c)
                            Gm, Gp = Gm * Sc, Gp * Sc
                    Gm, Gp = rule(Gm, 0), rule(Gp, 1)
                Xv = rule(Sv * _apply(H[y][0], U[y]), 0)
                W = _apply(H[y][0], Xv)
                Nn = _dot(Gm, W)
                Dd = _dot(Gp, S(y))
            km, kp = count
            with np.errstate(all="ignore"):
                r = np.where(Dd == 0.0, 0.0, Nn / Dd)
            for n in range(int(max((km - kp).max(), 0))):
                r = np.where(km - kp > n, r * R.TINY, r)
            for n in range(int(max((kp - km).max(), 0))):
                r = np.where(kp - km > n, r * R.SCALE, r)
            cat_rho[k, q], cat_km[k, q], cat_kp[k, q] = r, km, kp
            mixed = mixed + post[k] * r
        rho[q] = mixed
    out.update(rho=rho, cat_rho=cat_rho, cat_km=cat_km, cat_kp=cat_kp)
    return out


# ---- the regrafted tree, for a brute-force evaluation -----------------------------------------------------------------------------------
def regrafted(nleaves, parent, v, y):
    """The tree after candidate (v, y), renumbered children before parents (the leaves keep their numbers, the inner nodes in
    post-order, the root last).  Returns (parent', spec): spec[e'] says where the matrix of the new tree's edge e' comes from:
    ("P", e) the given tree's own, ("half", y) Ph_y, ("joined", p, s) the product P_p P_s of a dissolved p and its remaining child."""
    par = [int(x) for x in parent]
    n = len(par)
    kids = children_of(parent)
    p = par[v]
    spec = {x: ("P", x) for x in range(n) if par[x] != ROOT}
    new = n
    par.append(par[y])
    spec[new] = ("half", y)
    par[y] = new
    spec[y] = ("half", y)
    par[v] = new
    gone = None
    if len(kids[p]) == 2:
        s = [c for c in kids[p] if c != v][0]
        assert par[p] != ROOT and y != s and y != p
        par[s] = par[p]
        spec[s] = ("joined", p, s)
        gone = p
        del spec[p]
    alive = [x for x in range(n + 1) if x != gone]
    below = {x: [] for x in alive}
    top = None
    for x in alive:
        if par[x] == ROOT:
            top = x
        else:
            below[par[x]].append(x)
    order = list(range(nleaves))

    def post(x):
        for c in below[x]:
            post(c)
        if x >= nleaves:
            order.append(x)

    post(top)
    assert len(order) == len(alive)
    number = {old: k for k, old in enumerate(order)}
    out = [ROOT] * len(order)
    out_spec = [None] * (len(order) - 1)
    for old, k in number.items():
        if par[old] != ROOT:
            out[k] = number[par[old]]
            out_spec[k] = spec[old]
    return np.array(out, np.uint32), out_spec


def regrafted_matrices(dim, ncat, nedges, P, Ph, spec):
    """The C ABI's P of the regrafted tree (category-major) from the given tree's P and Ph."""
    parts = []
    Xall = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    Hall = np.asarray(Ph, np.float64).reshape(ncat, nedges * dim * dim)
    for k in range(ncat):
        X, H = R.unpack(Xall[k], nedges, 1, dim), R.unpack(Hall[k], nedges, 1, dim)
        mats = []
        for s in spec:
            mats.append([X[s[1]][0] if s[0] == "P" else H[s[1]][0] if s[0] == "half" else X[s[1]][0] @ X[s[2]][0]])
        parts.append(R.pack(np.array(mats)))
    return np.concatenate(parts)


def brute_log_rho(dim, nleaves, parent, rows, pi, w, P, Ph, v, y, own=None):
    """log of sum_k w_k L'_k / sum_k w_k L_k per site from two full evaluations: the regrafted tree's and the tree's own (`own`: the
    latter's result, where the caller has it)."""
    ncat, nedges = len(w), len(parent) - 1
    if own is None:
        own = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    parent2, spec = regrafted(nleaves, parent, v, y)
    there = G.evaluate(dim, nleaves, parent2, rows, pi, w, regrafted_matrices(dim, ncat, nedges, P, Ph, spec), derivs=False)
    with np.errstate(all="ignore"):
        return R.site_lnl(there["site_l"], there["site_k"]) - R.site_lnl(own["site_l"], own["site_k"])


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------------
TREES = dict(N.TREES)
_cases = {}


def half_matrices(dim, ncat, nedges, tree, rng):
    if tree == "caterpillar96":
        return R.pack(rng.uniform(0.03, 0.07, (ncat * nedges, 1, dim, dim)))
    H = rng.uniform(0.01, 1.0, (ncat * nedges, dim, dim))
    H /= H.sum(axis=2, keepdims=True)
    return R.pack(H[:, None])


def make_case(dim, ncols, tree, ncat, which="all", radius=MAXPATH, want=True):
    """A seeded case and its expectation, computed once per process: the inputs of treelik_nni_ref.make_case (its rows, pi, P, w), Ph
    drawn the same way, and the candidates: "all" within `radius` in the lister's order, "one" the first alone, "shuffled" all of them
    in a seeded order with the first three repeated at the end, or an array of rows (v, y)."""
    key = (dim, ncols, tree, ncat, which if isinstance(which, str) else np.asarray(which).tobytes(), radius)
    if key in _cases and (_cases[key]["want"] is not None or not want):
        return _cases[key]
    if tree in N.OWN_DRAW:
        base = N.make_case(dim, ncols, tree, ncat, "one")
    else:
        base = A.make_case(dim, ncols, tree, ncat)
    nleaves, parent, rows, pi, P, w = base["nleaves"], base["parent"], base["rows"], base["pi"], base["P"], base["w"]
    rng = np.random.default_rng(23000 + 1000 * dim + 7 * ncols + 13 * ncat + sum(map(ord, tree)))
    Ph = half_matrices(dim, ncat, len(parent) - 1, tree, rng)
    if isinstance(which, str):
        cand = candidates(nleaves, parent, radius)
        if which == "one":
            cand = cand[:1]
        elif which == "shuffled":
            order = np.random.default_rng(99 + dim + ncols).permutation(len(cand))
            cand = np.concatenate([cand[order], cand[:3]])
        else:
            assert which == "all"
    else:
        cand = np.asarray(which, np.uint32).reshape(-1, 2)
    case = dict(dim=dim, nleaves=nleaves, parent=parent, rows=rows, pi=pi, w=w, P=P, Ph=Ph, tree=tree, ncat=ncat, cand=cand,
                want=evaluate(dim, nleaves, parent, rows, pi, w, P, Ph, cand) if want else None)
    _cases[key] = case
    return case
