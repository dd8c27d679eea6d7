"""The independent statement of BioNJ's join record in numpy float64 (reference src/TreeNJ.cpp:132-281 as the host loop
bionj_joins_host restates it), and the helpers the tests of pgm_bionj / pgm_bionj_multi share (tests/test_cpu_bionj.py,
tests/test_gpu_bionj.py).

Elementwise numpy operations only (add, subtract, multiply, divide, comparisons, where), so every value has the bits of the scalar
statement; the two order-sensitive sums are spelled out: the column sums in the association of Eigen's vectorised reduction
(vectorised here ACROSS columns, grouped by the parity of their first aligned element), and vsum as np.add.accumulate, which adds
in index order.  The joined pair is np.argmin over the column-major flattening of the criterion with the diagonal at +inf: the
first minimum, row index fastest."""
import numpy as np

MIN_DIST, MIN_VAR = 1e-4, 1e-5
JOIN_DTYPE = np.dtype([("index1", "<u4"), ("index2", "<u4"), ("dist1", "<f8"), ("dist2", "<f8")])   # pgm_bionj_join, 24 bytes


def _clamp_low(x, lo):
    return np.where(x < lo, lo, x)   # std::max(x, lo)


def column_sums(R):
    """Sum of every column of the dim x dim matrix R as eigen_column_sum adds it (dim >= 4)."""
    dim = R.shape[0]
    assert dim >= 4
    out = np.empty(dim)
    for start in (0, 1):
        cols = np.array([j for j in range(dim) if ((j * dim) & 1) == start], dtype=np.int64)
        if cols.size == 0:
            continue
        X = R[:, cols]
        end2 = start + ((dim - start) // 4) * 4
        end = start + ((dim - start) // 2) * 2
        a0, a1, b0, b1 = X[start].copy(), X[start + 1].copy(), X[start + 2].copy(), X[start + 3].copy()
        for k in range(start + 4, end2, 4):
            a0 = a0 + X[k]
            a1 = a1 + X[k + 1]
            b0 = b0 + X[k + 2]
            b1 = b1 + X[k + 3]
        a0 = a0 + b0
        a1 = a1 + b1
        if end > end2:
            a0 = a0 + X[end2]
            a1 = a1 + X[end2 + 1]
        res = a0 + a1
        for k in range(0, start):
            res = res + X[k]
        for k in range(end, dim):
            res = res + X[k]
        out[cols] = res
    return out


def bionj_joins(D, V):
    """(joins, final_d, info) of the n x n matrices D, V (n >= 4; entry (i, j) at [i, j]); the inputs are not modified.
    joins: array of JOIN_DTYPE, n - 3 records; final_d: 3 x 3; info: how many joins clamped lambda to 0 and to 1, and under
    "lambda" the unclamped lambda of every join (NaN where the host takes 0.5)."""
    D = np.array(D, dtype=np.float64)
    V = np.array(V, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and V.shape == (n, n) and n >= 4
    D = _clamp_low(D, MIN_DIST)
    V = _clamp_low(V, MIN_VAR)
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(V, 0.0)
    act = np.arange(n)
    joins = np.zeros(n - 3, dtype=JOIN_DTYPE)
    info = dict(lambda_at_0=0, lambda_at_1=0, **{"lambda": np.full(n - 3, np.nan)})
    fresh = -1
    with np.errstate(all="ignore"):
        for step, dim in enumerate(range(n, 3, -1)):
            if fresh >= 0:   # the row / column the previous join wrote, from its column
                af = act[fresh]
                others = act[np.arange(dim) != fresh]
                d = _clamp_low(D[others, af], MIN_DIST)
                v = _clamp_low(V[others, af], MIN_VAR)
                D[others, af] = d
                D[af, others] = d
                V[others, af] = v
                V[af, others] = v
            R = D[np.ix_(act, act)]
            sums = column_sums(R)
            f = np.float64(0.5) / (np.float64(dim) - np.float64(2.0))
            q = 0.5 * R - f * (sums[None, :] + sums[:, None])   # q[row, col]
            np.fill_diagonal(q, np.inf)
            flat = q.T.reshape(-1)   # column-major: col * dim + row
            k = int(np.argmin(flat))
            if flat[k] < np.inf:
                index1, index2 = k // dim, k % dim   # (col, row)
            else:
                index1 = index2 = 0
            if index2 < index1:
                index1, index2 = index2, index1
            a1, a2 = act[index1], act[index2]
            d12 = D[a1, a2]
            dist1 = (d12 + (sums[index1] - sums[index2]) / (np.float64(dim) - 2.0)) / 2.0
            dist1 = MIN_DIST if dist1 < MIN_DIST else dist1
            dist1 = d12 if d12 < dist1 else dist1
            dist2 = D[a2, a1] - dist1
            dist2 = MIN_DIST if dist2 < MIN_DIST else dist2
            diffs = V[a2, act] - V[a1, act]
            vsum = np.add.accumulate(np.concatenate([[0.0], diffs]))[-1]
            v12 = V[a1, a2]
            lam = np.float64(0.5) + vsum / (np.float64(2 * (dim - 2)) * v12)
            info["lambda"][step] = lam
            if np.isnan(lam):
                lam = np.float64(0.5)
            else:   # std::min(std::max(0.0, lambda), 1.0)
                info["lambda_at_0"] += int(lam < 0.0)
                info["lambda_at_1"] += int(lam > 1.0)
                lam = lam if np.float64(0.0) < lam else np.float64(0.0)
                lam = np.float64(1.0) if np.float64(1.0) < lam else lam
            keep = np.arange(dim) != index2
            rest = act[keep]
            nd = lam * (D[a1, rest] - dist1) + (1.0 - lam) * (D[a2, rest] - dist2)
            nv = lam * V[a1, rest] + (1.0 - lam) * V[a2, rest] - lam * (1.0 - lam) * v12
            own = rest == a1
            nd = np.where(own, 0.0, nd)
            nv = np.where(own, 0.0, nv)
            D[a1, rest] = nd
            D[rest, a1] = nd
            V[a1, rest] = nv
            V[rest, a1] = nv
            act = rest
            fresh = index1
            joins[step] = (index1, index2, dist1, dist2)
    return joins, D[np.ix_(act, act)].copy(), info


# ---- the driver's dumps -----------------------------------------------------------------------------------------------------
def read_dist_dump(path):
    """[(D, V)] of a --dump_dist file: per matrix the int32 dimension, then dim^2 distances and dim^2 variances (row-major)."""
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        n = int(np.frombuffer(raw, "<i4", 1, o)[0])
        o += 4
        D = np.frombuffer(raw, "<f8", n * n, o).reshape(n, n).copy()
        o += 8 * n * n
        V = np.frombuffer(raw, "<f8", n * n, o).reshape(n, n).copy()
        o += 8 * n * n
        out.append((D, V))
    return out


def read_joins_dump(path):
    """[(n, joins, final_d)] of a --dump_joins file: per tree the int32 n, max(n - 3, 0) records (two int32, two doubles), nine doubles."""
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        n = int(np.frombuffer(raw, "<i4", 1, o)[0])
        o += 4
        nj = max(n - 3, 0)
        joins = np.frombuffer(raw, JOIN_DTYPE, nj, o).copy()
        o += JOIN_DTYPE.itemsize * nj
        final_d = np.frombuffer(raw, "<f8", 9, o).reshape(3, 3).copy()
        o += 72
        out.append((n, joins, final_d))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the matrices of tests/test_gpu_bionj.py -------------------------------------------------------------------------------
KINDS = ["random", "asym", "ties", "ints", "tiny", "lambda"]


def matrices(kind, n, seed=0):
    """(D, V) of one kind: random symmetric D in (0, 2) with V in (1e-3, 1); the same with a 1-ulp asymmetry on D and V; all
    off-diagonal D equal to 1; small-integer D (both: mass exact ties); entries below MIN_DIST / MIN_VAR; V rows scaled by 100 or
    by 1 (not symmetric: lambda leaves [0, 1] on either side when a join pairs a scaled row with an unscaled one)."""
    rng = np.random.default_rng(1000 * n + seed + 7 * KINDS.index(kind))
    U = rng.uniform(0.0, 2.0, (n, n))
    D = np.triu(U, 1) + np.triu(U, 1).T
    W = rng.uniform(1e-3, 1.0, (n, n))
    V = np.triu(W, 1) + np.triu(W, 1).T
    if kind == "asym":
        D = np.where(rng.random((n, n)) < 0.5, np.nextafter(D, 4.0), D)
        V = np.where(rng.random((n, n)) < 0.5, np.nextafter(V, 4.0), V)
    elif kind == "ties":
        D = np.ones((n, n))
    elif kind == "ints":
        I = rng.integers(1, 4, (n, n)).astype(np.float64)
        D = np.triu(I, 1) + np.triu(I, 1).T
    elif kind == "tiny":
        D = np.where(rng.random((n, n)) < 0.3, D * 1e-5, D)   # (not symmetric either)
        V = np.where(rng.random((n, n)) < 0.3, V * 1e-6, V)
    elif kind == "lambda":
        V = V * np.where(rng.random(n) < 0.5, 100.0, 1.0)[:, None]
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(V, 0.0)
    return np.ascontiguousarray(D), np.ascontiguousarray(V)
