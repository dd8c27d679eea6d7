"""The nearest-neighbour interchanges of `pgmsa --ml_nni_opt`, each at a trial length of its own central edge, stated independently of
the C++ and the kernels (include/pgm_hip.h: pgm_tree_nni_edge), in numpy float64, vectorised over the sites only.

site_l, site_k and post are treelik_rates_ref.evaluate's without derivatives; the walk of a category is treelik_nni_ref.walk; the four
pieces around a candidate's edge are formed as treelik_nni_ref.evaluate forms them, the neighbour's W three times from the candidate's
own matrices.  Every sum is a Python loop ascending from 0.0 with one multiply and one add per term.  optimise() restates
ml_nni_edge_lengths (host/treelik_nni.cpp) in plain Python over any function that gives the matrices of a vector of trial lengths;
rational_matrices is such a function in + - * / alone, so that the stand-alone host program can be compared with it bit for bit.
The seeded cases serve tests/test_cpu_mlnniopt.py and tests/test_gpu_mlnniopt.py."""
import math

import numpy as np

import treelik_nni_ref as N
import treelik_rates_ref as G
import treelik_ref as R
from treelik_ref import _apply, _dot, _rescale, children_of

T_MIN, T_MAX = R.T_MIN, R.T_MAX


def evaluate(dim, nleaves, parent, rows, pi, w, P, cand, Pc):
    """pgm_tree_nni_edge.  cand: rows (v, a, c); Pc: ncat x ncand x 3 x dim x dim, the C ABI's flat array.  Returns a dict: site_l, site_k,
    post, rho (ncand x ncols), d1, d2 (ncand), the per-site g, h (ncand x ncols), and whether D == 0 occurred (any_d0)."""
    parent = np.asarray(parent, np.uint32)
    rows = np.asarray(rows, np.int8)
    pi = np.asarray(pi, np.float64)
    w = np.asarray(w, np.float64)
    cand = np.asarray(cand, np.int64).reshape(-1, 3)
    ncat, nedges, ncols, ncand = len(w), len(parent) - 1, rows.shape[1], len(cand)
    root = len(parent) - 1
    kids = children_of(parent)
    Xall = np.asarray(P, np.float64).reshape(ncat, nedges * dim * dim)
    Zall = np.asarray(Pc, np.float64).reshape(ncat, ncand * 3 * dim * dim)
    out = G.evaluate(dim, nleaves, parent, rows, pi, w, P, derivs=False)
    post = out["post"]
    walks = []
    for k in range(ncat):
        X = R.unpack(Xall[k], nedges, 1, dim)
        L, kk, U, O = N.walk(dim, nleaves, parent, rows, pi, X)
        walks.append((X, U, O, R.unpack(Zall[k], ncand, 3, dim)))
    rho, g, h = np.zeros((ncand, ncols)), np.zeros((ncand, ncols)), np.zeros((ncand, ncols))
    any_d0 = False
    for q, (v, a, c) in enumerate(cand):
        v, a, c = int(v), int(a), int(c)
        u = int(parent[v])
        mixed, Gs, Qs = np.zeros(ncols), np.zeros(ncols), np.zeros(ncols)
        for k in range(ncat):
            X, U, O, Z = walks[k]
            S = lambda x: _apply(X[x][0], U[x])
            Rv = N._base(dim, ncols, pi, X, O, u, root)
            for sib in kids[u]:
                if sib != v and sib != c:
                    Rv = Rv * S(sib)
            T = None
            for b in kids[v]:
                if b != a:
                    T = S(b) if T is None else T * S(b)
            Sa, Sc = S(a), S(c)
            XD, hx = _rescale(T * Sa)
            YD, hy = _rescale(Rv * Sc)
            kD = hx.astype(np.int32) + hy.astype(np.int32)
            D = _dot(YD, _apply(X[v][0], XD))
            XN, hx = _rescale(T * Sc)
            YN, hy = _rescale(Rv * Sa)
            kN = hx.astype(np.int32) + hy.astype(np.int32)
            any_d0 = any_d0 or bool(np.any(D == 0.0))
            rs = []
            for x in range(3):
                Nx = _dot(YN, _apply(Z[q][x], XN))
                with np.errstate(all="ignore"):
                    r = np.where(D == 0.0, 0.0, Nx / D)
                for n in range(int(max((kN - kD).max(), 0))):
                    r = np.where(kN - kD > n, r * R.TINY, r)
                for n in range(int(max((kD - kN).max(), 0))):
                    r = np.where(kD - kN > n, r * R.SCALE, r)
                rs.append(r)
            mixed = mixed + post[k] * rs[0]
            Gs = Gs + post[k] * rs[1]
            Qs = Qs + post[k] * rs[2]
        with np.errstate(all="ignore"):
            gq = np.where(mixed == 0.0, 0.0, Gs / mixed)
            hq = np.where(mixed == 0.0, 0.0, Qs / mixed - gq * gq)
        rho[q], g[q], h[q] = mixed, gq, hq
    out.update(rho=rho, g=g, h=h, d1=R.chunk_sums(g), d2=R.chunk_sums(h), any_d0=any_d0)
    return out


# ---- the optimiser ----------------------------------------------------------------------------------------------------------------------
def clamp(x):
    return T_MIN if x < T_MIN else T_MAX if x > T_MAX else x


def optimise(case, matrices, lengths, rounds, group=None):
    """ml_nni_edge_lengths: matrices(t) gives Pc for the trial lengths t (a list).  group: candidates per evaluate() call (None: all).
    Returns (t_opt, gain_opt, rho rows at t_opt) and the trial lengths of every round."""
    cand = np.asarray(case["cand"]).reshape(-1, 3)
    ncand = len(cand)
    group = group or ncand
    t_best, gain_best, b1, b2, lam = [0.0] * ncand, [0.0] * ncand, [0.0] * ncand, [0.0] * ncand, [1.0] * ncand
    rows_best = np.zeros((ncand, case["rows"].shape[1]))
    trials = []
    for rnd in range(rounds + 1):
        trial = []
        for q in range(ncand):
            if rnd == 0:
                trial.append(float(lengths[int(cand[q][0])]))
                continue
            t = t_best[q]
            target = t - b1[q] / b2[q] if b2[q] < 0 else 2 * t if b1[q] > 0 else t / 2
            trial.append(clamp(t + lam[q] * (clamp(target) - t)))
        trials.append(trial)
        rho, d1, d2 = [], [], []
        for q0 in range(0, ncand, group):
            sl = slice(q0, min(ncand, q0 + group))
            o = evaluate(case["dim"], case["nleaves"], case["parent"], case["rows"], case["pi"], case["w"], case["P"], cand[sl], matrices(trial[sl]))
            rho.append(o["rho"]); d1.append(o["d1"]); d2.append(o["d2"])
        rho, d1, d2 = np.concatenate(rho), np.concatenate(d1), np.concatenate(d2)
        gain = N.gain(rho)
        for q in range(ncand):
            if rnd == 0 or gain[q] > gain_best[q]:
                t_best[q], gain_best[q], b1[q], b2[q], lam[q] = trial[q], float(gain[q]), float(d1[q]), float(d2[q]), 1.0
                rows_best[q] = rho[q]
            else:
                lam[q] = lam[q] * 0.5
    return np.array(t_best), np.array(gain_best), rows_best, trials


def rational_matrices(A, B):
    """A family of matrices in + - * / alone, per category k: Z(t) = (A_k + t B_k) / (1 + t) and its first and second derivative by t,
    (B_k - A_k) / ((1 + t) (1 + t)) and -2 (B_k - A_k) / (((1 + t) (1 + t)) (1 + t)).  A, B: ncat x dim x dim row-stochastic, so Z(t) is.
    Returns the function optimise() takes; tests/native/treelik_nni_edge_test.cpp states the same arithmetic."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)

    def matrices(t):
        out = np.zeros((A.shape[0], len(t), 3) + A.shape[1:])
        for k in range(A.shape[0]):
            for q, tq in enumerate(t):
                one = 1.0 + tq
                sq = one * one
                out[k, q, 0] = (A[k] + tq * B[k]) / one
                out[k, q, 1] = (B[k] - A[k]) / sq
                out[k, q, 2] = (-2.0 * (B[k] - A[k])) / (sq * one)
        return R.pack(out.reshape((-1, 3) + A.shape[1:]))

    return matrices


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------
_cases = {}


def draw_pc(rng, ncat, ncand, dim, tree):
    if tree == "caterpillar96":
        X = rng.uniform(0.03, 0.07, (ncat * ncand, 3, dim, dim))
    else:
        P0 = rng.uniform(0.01, 1.0, (ncat * ncand, dim, dim))
        P0 /= P0.sum(axis=2, keepdims=True)
        X = np.stack([P0, rng.normal(0, 0.5, (ncat * ncand, dim, dim)), rng.normal(0, 1.0, (ncat * ncand, dim, dim))], axis=1)
    return R.pack(X)


def own_blocks(case, Pc):
    """Pc with the P block of every (category, candidate) replaced by P_v of that category: rho is then pgm_tree_nni's."""
    dim, ncat, nedges, cand = case["dim"], case["ncat"], len(case["parent"]) - 1, np.asarray(case["cand"]).reshape(-1, 3)
    out = np.array(Pc, np.float64).reshape(ncat, len(cand), 3, dim * dim)
    P = np.asarray(case["P"]).reshape(ncat, nedges, dim * dim)
    for q, (v, _, _) in enumerate(cand):
        out[:, q, 0, :] = P[:, int(v), :]
    return out.reshape(-1)


def with_pc(base, Pc, tree=None):
    case = dict(base, Pc=Pc)
    if tree:
        case["tree"] = tree
    case["nni_want"] = base["want"]
    case["want"] = evaluate(base["dim"], base["nleaves"], base["parent"], base["rows"], base["pi"], base["w"], base["P"], base["cand"], Pc)
    return case


def make_case(dim, ncols, tree, ncat, which="all", own=False):
    """treelik_nni_ref.make_case's case with drawn matrices of the candidates' own (row-stochastic P, signed P' and P''; the caterpillar:
    every entry in [0.03, 0.07]).  own: the P blocks are the tree's own P_v.  Computed once per process."""
    key = (dim, ncols, tree, ncat, which, own)
    if key in _cases:
        return _cases[key]
    base = N.make_case(dim, ncols, tree, ncat, which)
    rng = np.random.default_rng(9100 + 1000 * dim + 7 * ncols + 13 * ncat + sum(map(ord, tree)) + len(base["cand"]))
    Pc = draw_pc(rng, ncat, len(base["cand"]), dim, tree)
    if own:
        Pc = own_blocks(base, Pc)
    _cases[key] = with_pc(base, Pc)
    return _cases[key]


def zeros_case():
    """Matrices with zeros on the balanced tree of 8, dim 4, 17 columns, 2 categories: category 0's column of state 1 of the edge above
    leaf 2 is zero, so the sites where leaf 2 has state 1 have L_0 == 0 and D == 0 there for every candidate (post_0 == 0); the
    matrices of candidates 3 and 4 are all zero, so their rho is 0 everywhere and g = h = 0."""
    key = "zeros"
    if key in _cases:
        return _cases[key]
    base = N.make_case(4, 17, "balanced8", 2)
    rows = base["rows"].copy()
    rows[2, 8] = 1
    rows[2, 9] = 1
    P = np.array(base["P"], np.float64).reshape(2, 14, 4, 4)   # [k][e][j][i]
    P[0, 2, 1, :] = 0.0
    P = P.reshape(-1)
    nb = dict(base, rows=rows, P=P, want=N.evaluate(4, 8, base["parent"], rows, base["pi"], base["w"], P, base["cand"]))
    rng = np.random.default_rng(4711)
    Pc = draw_pc(rng, 2, 12, 4, "balanced8").reshape(2, 12, 3 * 16)
    Pc[:, 3:5, :] = 0.0
    case = with_pc(nb, Pc.reshape(-1), tree="balanced8, zeros")
    w = case["want"]
    assert w["any_d0"] and np.all(w["rho"][3:5] == 0.0) and np.all(w["g"][3:5] == 0.0) and np.all(w["h"][3:5] == 0.0)
    assert np.all(w["post"][0][8:10] == 0.0) and not np.any(np.isnan(w["rho"])) and np.all(np.isfinite(w["d1"])) and np.all(np.isfinite(w["d2"]))
    _cases[key] = case
    return case
