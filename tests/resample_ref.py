"""The sums over resampled columns and the branch-support statistics of `pgmsa --ml_tree --ml_support`, stated independently of the C++
and the kernels (include/pgm_hip.h: pgm_resampled_sums), in numpy float64 and plain Python.

sums: one vectorised addition per step k, so every out entry is the chain 0.0 + x[q, cols[r, 0]] + x[q, cols[r, 1]] + ... in that order.
support: the definitions of DESIGN 3.21 over math.log (the C library's, as treelik_nni_ref.gain) of treelik_nni_ref's rho.  The seeded
cases serve tests/test_cpu_mlsupport.py and tests/test_gpu_mlsupport.py."""
import math

import numpy as np

import treelik_nni_ref as N
from treelik_ref import children_of

MASK = (1 << 64) - 1
T = 64   # the kernel's q-tile (PGM_RESAMPLE_T)


def sums(x, cols):
    """pgm_resampled_sums: x nrow x ncols, cols nrep x ncols -> nrow x nrep."""
    x = np.asarray(x, np.float64)
    cols = np.asarray(cols, np.int64)
    acc = np.zeros((x.shape[0], cols.shape[0]))
    with np.errstate(invalid="ignore"):
        for k in range(cols.shape[1]):
            acc = acc + x[:, cols[:, k]]
    return acc


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def columns(nrep, ncols, seed):
    """--bootstrap's replicate columns: cols[r][c] = splitmix64() % ncols, c ascending, replicates in order, one stream."""
    out = np.zeros((nrep, ncols), np.uint32)
    state = seed & MASK
    for r in range(nrep):
        for c in range(ncols):
            state, z = splitmix64(state)
            out[r, c] = z % ncols
    return out


def supported(nleaves, parent):
    """The supported nodes, ascending, and their candidates (v, a, c): a in child order, then c in child order."""
    kids = children_of(parent)
    root = len(parent) - 1
    nodes, cand = [], []
    for v in range(nleaves, root):
        u = int(parent[v])
        if u == root and len(kids[u]) == 2:
            continue
        nodes.append(v)
        for a in kids[v]:
            for c in kids[u]:
                if c != v:
                    cand.append((v, a, c))
    return nodes, np.array(cand, np.uint32).reshape(-1, 3)


def log_rho(rho):
    return np.array([[math.log(v) if v > 0.0 else -math.inf if v == 0.0 else math.nan for v in row] for row in rho]).reshape(np.shape(rho))


def statistics(nodes, cand, rho, cols):
    """Per supported node (node, candidates, alrt, sh_hits, rell_hits) from the candidates' rho (ncand x ncols) and the replicates' columns."""
    nrep = len(cols)
    gain = N.gain(rho)
    D = sums(log_rho(rho), cols)
    out = []
    for v in nodes:
        mine = [q for q in range(len(cand)) if int(cand[q][0]) == v]
        C = [q for q in mine if gain[q] != -math.inf]
        if not C:
            out.append((v, len(mine), math.inf, nrep, nrep))
            continue
        d_obs = -max(float(gain[q]) for q in C)
        mean = {}
        for q in C:
            total = 0.0
            for r in range(nrep):
                total = total + float(D[q, r])
            mean[q] = total / nrep
        sh = rell = 0
        for r in range(nrep):
            e = sorted([0.0] + [float(D[q, r]) - mean[q] for q in C])
            gap = e[-1] - e[-2]
            if d_obs > 0 and gap < d_obs:
                sh += 1
            if all(float(D[q, r]) <= 0.0 for q in C):
                rell += 1
        out.append((v, len(mine), 2.0 * d_obs, sh, rell))
    return out


# ---- seeded cases of the sums ------------------------------------------------------------------------------------------------------------
NROWS = (1, 2, 63, 64, 65, T - 1, T, T + 1, 4 * T + 1)
NCOLS = (1, 2, 17, 257, 2891)   # (the transpose's tile is 32 x 32: 257 is past it; 2891 is the width of DESIGN 3.21's largest family, odd)
NREPS = (1, 2, 63, 64, 65, 1000)
# every value of each dimension with small values of the others, and the corners
SHAPES = list(dict.fromkeys([(nrow, 17, 5) for nrow in NROWS] + [(65, ncols, 3) for ncols in NCOLS] + [(3, 17, nrep) for nrep in NREPS]
                            + [(4 * T + 1, 257, 65), (T + 1, 2, 1000), (1, 1, 1), (70001, 3, 2)]))
KINDS = ("random", "one column", "identity", "minus infinity", "mixed magnitude")

_cases = {}


def make_case(nrow, ncols, nrep, kind="random"):
    """(x, cols, want), computed once per process and never changed."""
    key = (nrow, ncols, nrep, kind)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(7000 + 31 * nrow + 7 * ncols + nrep + sum(map(ord, kind)))
    x = -rng.exponential(1.0, (nrow, ncols)) + 0.3
    cols = rng.integers(0, ncols, (nrep, ncols)).astype(np.uint32)
    if kind == "one column":
        cols[:] = ncols - 1
    elif kind == "identity":
        cols[:] = np.arange(ncols, dtype=np.uint32)[None, :]
    elif kind == "minus infinity":
        x[rng.random((nrow, ncols)) < 0.02] = -np.inf
        x[nrow // 2, :] = -np.inf
    elif kind == "mixed magnitude":   # 1e-300 .. 1e300 of both signs: any other order of the additions shows
        x = rng.choice([-1.0, 1.0], (nrow, ncols)) * 10.0 ** rng.uniform(-300, 300, (nrow, ncols))
    else:
        assert kind == "random"
    x.setflags(write=False); cols.setflags(write=False)
    want = sums(x, cols)
    want.setflags(write=False)
    _cases[key] = (x, cols, want)
    return _cases[key]


def bad_calls():
    """What the entry refuses, as (x, cols) of a valid 3 x 5 x 2 call changed: a cols entry >= ncols (the first, the last, the largest)."""
    x, cols, _ = make_case(3, 5, 2)
    out = []
    for at, v in (((0, 0), 5), ((1, 4), 5), ((1, 2), 0xFFFFFFFF)):
        c = np.array(cols)
        c[at] = v
        out.append((x, c))
    return out
