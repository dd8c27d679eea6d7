"""The independent statement of the ML distance estimator for a general generator Q (no eigen form), in numpy float64, and the
helpers the tests of pgm_mldist_general_kernel share (tests/test_gpu_mldist_general.py, tests/test_gpu_mldist_codon_e2e.py,
tests/test_cpu_mldist_general.py), and the models and pairs of the eigen-form kernel's dims-and-rounds test (tests/test_gpu_dist.py)
and of its CPU companion.

P(d) = exp(Q d) by the recipe of host/model_factory.cpp's expm: scale by 2^-s (s from the 1-norm rule), 20 Taylor terms, s
squarings.  Around it the Newton iteration of DistanceFactoryML.h:66-190 (computeDistance / computeMLDist).  The matrix products
and the sums are numpy's own (BLAS association, pairwise sums): the statement fixes the values, not their last bits."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "prographmsa_amd", "host", "data")

# the constants of DistanceFactoryML.cpp:5-32 and the defaults of the driver's options (--codon: max_dist = cutoff_dist = 5)
CODON_PAR = dict(dist_max=5.2, var_max=5e3, var_min=1e-5, cutoff_dist=5.0, min_dist=0.05, max_dist=5.0, indel_rate=0.0093359375)
AA_PAR = dict(dist_max=2.2, var_max=1e3, var_min=1e-5, cutoff_dist=2.2, min_dist=0.05, max_dist=2.2, indel_rate=0.0093359375)


def expm_taylor(A):
    """exp(A) as the host's expm evaluates it; returns (E, s)."""
    n = A.shape[0]
    norm = float(np.abs(A).sum(axis=0).max())
    s = 0
    while norm > 0.5:
        norm *= 0.5
        s += 1
    A = A * 2.0 ** -s
    E, term = np.eye(n), np.eye(n)
    for k in range(1, 21):
        term = (term @ A) * (1.0 / k)
        E = E + term
    for _ in range(s):
        E = E @ E
    return E, s


def estimate(Q, counts, gaps, seqlen, par, mldist=1, mldist_gap=0):
    """One pair.  Q: n x n generator (Q[i, j] the entry the C ABI stores at i + n j); counts: n x n with counts[s1, s2] the entry at
    s1 + n s2.  Returns (dist, var, info); info names the branches the pair took."""
    info = dict(newton=0, squarings=[], exit="none")
    c = np.asarray(counts, np.float64)
    ident, total = float(np.trace(c)), float(c.sum())
    with np.errstate(all="ignore"):
        dist0 = 1.0 - ident / total if total else float("nan")
        if mldist or mldist_gap:
            if total == 0 or dist0 > 0.85:
                dist = dist0 = par["dist_max"]; var = par["var_max"]; info["start"] = "dist_max"
            else:
                dist = dist0 = -np.log(1.0 - dist0 - 0.2 * dist0 * dist0); var = dist / total; info["start"] = "pdist"
            if total > 0 and ident != total:
                var0 = var
                lo, hi, delta, it = 0.0, np.inf, 1.0, 0
                while abs(delta) > 1e-5:
                    if it > 20:
                        if hi == np.inf:
                            dist, var = par["dist_max"], par["var_max"]; info["exit"] = "maxiter_unbracketed"
                        else:
                            dist, var = dist0, var0; info["exit"] = "maxiter_bracketed"
                        break
                    dm = max(0.0, dist)
                    if dist != dist:
                        dm = 5.2
                    dm = max(min(dm, par["max_dist"]), par["min_dist"])
                    P, s = expm_taylor(Q * dm)
                    info["squarings"].append(s)
                    P1 = Q @ P
                    P2 = Q @ P1
                    f = float(np.sum(c * P1 / P))
                    ff = float(np.sum(c * (P2 * P - P1 * P1) / (P * P)))
                    if mldist_gap:
                        grate = par["indel_rate"] * seqlen * dist
                        f += (-grate + gaps) / dist
                        ff += -float(gaps) / (dist * dist)
                    var = -1.0 / ff
                    if f > 0:
                        lo = max(lo, dist)
                    else:
                        hi = min(hi, dist)
                    new = dist - f / ff
                    if not (new < hi and new > lo):
                        new = ((dist * 3 if hi == np.inf else hi) + lo) / 2.0
                    delta = 1.0 - new / dist
                    dist = new
                    it += 1
                info["newton"] = it
                if info["exit"] == "none":
                    info["exit"] = "converged"
        else:
            if total == 0:
                dist = dist0 = 1.0; var = par["var_max"]
            else:
                dist = dist0; var = dist0 / total
        if not dist < par["dist_max"]:
            dist, var = par["dist_max"], par["var_max"]
        if dist > par["cutoff_dist"]:
            dist = par["cutoff_dist"]
        if var < par["var_min"]:
            var = par["var_min"]
        if not var < par["var_max"]:
            var = par["var_max"]
    return float(dist), float(var), info


def estimate_batch(Q, counts, gaps, seqlen, par, mldist=1, mldist_gap=0):
    """counts: (npairs, n * n) in the C ABI's layout.  Returns (dist, var, [info])."""
    n = Q.shape[0]
    out = [estimate(Q, np.asarray(counts[p]).reshape(n, n, order="F"), int(gaps[p]), float(seqlen[p]), par, mldist, mldist_gap) for p in range(len(gaps))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), [o[2] for o in out]


def rel_diff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


# ---- models -------------------------------------------------------------------------------------------------------------
def read_qmat(path):
    """A rate matrix file of host/data: `rows cols`, then the entries column-major."""
    tok = open(path).read().split()
    n = int(tok[0])
    assert int(tok[1]) == n
    return np.array([float(x) for x in tok[2:2 + n * n]]).reshape(n, n, order="F")


def normalised(Q, freqs):
    """ModelFactory::normalise: diagonal reset to minus the row sums, then the rate -sum(freqs_i Q_ii) scaled to 1."""
    Q = Q.copy()
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(freqs @ np.diag(Q))


def shipped_model(name):
    """The generator the driver builds from host/data/<name> (ModelFactory's constructor): frequencies = the null vector of Q^T
    normalised to sum 1, then normalised()."""
    Q = read_qmat(os.path.join(DATA, name))
    n = Q.shape[0]
    A = Q.T.copy()
    A[n - 1, :] = 1.0
    b = np.zeros(n); b[n - 1] = 1.0
    return normalised(Q, np.linalg.solve(A, b))


def random_generator(n, seed):
    """Positive off-diagonals, rows summing to zero, no reversibility imposed; mean rate 1 under uniform weights."""
    rng = np.random.default_rng(seed)
    Q = rng.gamma(0.7, 1.0, (n, n)) + 0.02
    return normalised(Q, np.full(n, 1.0 / n))


def counts_at(Q, d, nsites, rng, identical=False):
    """The count matrix of nsites columns of a pair at distance d under Q, as an n x n array counts[s1, s2]."""
    n = Q.shape[0]
    c = np.zeros((n, n), np.int32)
    if nsites == 0:
        return c
    a = rng.integers(0, n, nsites)
    if identical:
        b = a
    else:
        P = np.clip(expm_taylor(Q * d)[0], 0, None)
        P /= P.sum(axis=1, keepdims=True)
        b = np.array([rng.choice(n, p=P[x]) for x in a])
    np.add.at(c, (a, b), 1)
    return c


# ---- the driver's dump (--dump_dist) ----------------------------------------------------------------------------------------
def read_dump(path):
    """[(D, V)] of a --dump_dist file: per matrix the int32 dimension, then dim^2 distances and dim^2 variances."""
    buf = open(path, "rb").read()
    mats, off = [], 0
    while off < len(buf):
        n = int(np.frombuffer(buf, np.int32, 1, off)[0]); off += 4
        d = np.frombuffer(buf, np.float64, n * n, off); off += 8 * n * n
        v = np.frombuffer(buf, np.float64, n * n, off); off += 8 * n * n
        mats.append((d, v))
    return mats


# ---- the inputs of the kernel test ------------------------------------------------------------------------------------------
# the driver's codon defaults (the clamp of parseDistance ends at 5), and a wide set: the clamp reaches the codon DIST_MAX of 5.2
# and starts at 0.001
WIDE_PAR = dict(CODON_PAR, min_dist=1e-3, max_dist=5.2, cutoff_dist=5.2)
NPAIRS = 257


def kernel_test_pairs(Q, seed):
    """257 pairs for one model: counts (npairs, n * n) int32 in the C ABI's layout, gaps, seqlen.  The first five hold the special
    pairs, so that the launches of 1 and 5 pairs see them too."""
    n = Q.shape[0]
    rng = np.random.default_rng(seed)
    cs = []
    cs.append(counts_at(Q, 0.4, 300, rng))                       # 0: an ordinary pair
    cs.append(counts_at(Q, 0.0, 200, rng, identical=True))       # 1: ident == total
    cs.append(np.zeros((n, n), np.int32))                        # 2: total == 0
    c = rng.integers(0, 3, (n, n)).astype(np.int32); np.fill_diagonal(c, 0); c[0, 1] += 1
    cs.append(c)                                                 # 3: p-distance 1 > 0.85 (start at DIST_MAX, no root: no upper bracket)
    c = counts_at(Q, 0.0, 2000, rng, identical=True).copy(); c[0, 1] += 1
    cs.append(c)                                                 # 4: one difference in 2001 columns (root below every clamp)
    dists = [0.02, 0.08, 0.15, 0.3, 0.6, 1.0, 1.6, 2.4, 3.5, 5.0]
    while len(cs) < NPAIRS:
        k = len(cs)
        cs.append(counts_at(Q, dists[k % len(dists)], int(rng.integers(30, 400)), rng))
    counts = np.ascontiguousarray(np.stack([c.reshape(-1, order="F") for c in cs]).astype(np.int32))
    gaps = rng.integers(0, 30, NPAIRS).astype(np.uint32)
    gaps[0] = 7
    seqlen = rng.uniform(50, 1200, NPAIRS)
    return counts, gaps, seqlen


# ---- the inputs of the eigen-form kernel's dims-and-rounds test (tests/test_gpu_dist.py) and of its CPU companion ------------
EIGEN_DIMS = (2, 4, 19, 20)
EIGEN_FLAGS = ((1, 0), (0, 1))
EIGEN_KINDS = ("near", "empty", "far", "identical", "saturated")
_eigen_cache = {}


def eigen_model(dim):
    """A random reversible model in eigen form, built as tests/test_gpu_dist.py builds its 20-state one: symmetric exchangeabilities
    times pi, normalised to rate 1, then numpy's eig.  Returns (Q, V, Vi, sigma)."""
    rng = np.random.default_rng(900 + dim)
    pi = rng.dirichlet(np.ones(dim) * 5)
    S = rng.gamma(0.5, 1.0, (dim, dim)); S = (S + S.T) / 2; np.fill_diagonal(S, 0)
    Q = S * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(1))
    Q /= -(pi * np.diag(Q)).sum()
    sig, V = np.linalg.eig(Q)
    assert np.all(sig.imag == 0) and np.all(V.imag == 0)
    sig, V = sig.real, V.real
    return Q, V, np.linalg.inv(V), sig


def eigen_ctypes_model(dim, flags, par=None):
    """pgm_mldist_model of eigen_model(dim) with the amino-acid constants; returns (model, the arrays it points into)."""
    import ctypes as C
    import prographmsa_amd as pg
    Q, V, Vi, sig = eigen_model(dim)
    keep = [np.asfortranarray(Q), np.asfortranarray(V), np.asfortranarray(Vi), np.ascontiguousarray(sig)]
    m = pg.pgm_mldist_model()
    m.dim = dim
    m.Q, m.V, m.Vi, m.sigma = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in keep]
    for k, v in (par or AA_PAR).items():
        setattr(m, k, v)
    m.mldist, m.mldist_gap = flags
    return m, keep


def eigen_pool(dim):
    """The distinct pairs of the test, by kind (computed once per dim): a dict kind -> (counts (m, n * n) int32 in the C ABI's
    layout, gaps, seqlen).  `near` / `far`: counts_at at distances 0.02 .. 0.3 / 0.5 .. 3; `empty`: no column; `identical`: only
    diagonal counts; `saturated`: p-distance above 0.85 (the start at DIST_MAX)."""
    if dim in _eigen_cache:
        return _eigen_cache[dim]
    Q = eigen_model(dim)[0]
    rng = np.random.default_rng(7000 + dim)
    cs = {k: [] for k in EIGEN_KINDS}
    for d in (0.02, 0.05, 0.1, 0.2, 0.3):
        for _ in range(6):
            cs["near"].append(counts_at(Q, d, int(rng.integers(60, 400)), rng))
    for d in (0.5, 0.8, 1.2, 2.0, 3.0):
        for _ in range(6):
            cs["far"].append(counts_at(Q, d, int(rng.integers(60, 400)), rng))
    for _ in range(4):
        cs["empty"].append(np.zeros((dim, dim), np.int32))
    for _ in range(6):
        cs["identical"].append(counts_at(Q, 0.0, int(rng.integers(1, 500)), rng, identical=True))
    for _ in range(6):
        c = rng.integers(1, 40, (dim, dim)).astype(np.int32)
        np.fill_diagonal(c, 0)
        c[0, 0] = int(rng.integers(0, 3))
        cs["saturated"].append(c)
    pool = {}
    for k in EIGEN_KINDS:
        m = len(cs[k])
        pool[k] = (np.ascontiguousarray(np.stack([c.reshape(-1, order="F") for c in cs[k]]).astype(np.int32)),
                   rng.integers(0, 30, m).astype(np.uint32), rng.uniform(50, 1200, m))
    _eigen_cache[dim] = pool
    return pool


def eigen_schedule(npairs, stride):
    """Which pool entry pair p of the launch is: (kind index, entry index) arrays.  `stride` is the number of pairs of one round of
    the grid (4 wavefronts x the blocks of the launch): pairs p and p + stride run on the same wavefront in consecutive rounds, and
    the kind advances by one from round to round, so they are always of different kinds."""
    p = np.arange(npairs)
    kind = (p % stride + p // stride) % len(EIGEN_KINDS)
    return kind, p // len(EIGEN_KINDS)


def eigen_pairs(dim, npairs, stride):
    """counts (npairs, n * n), gaps, seqlen and the kind of every pair, drawn from the pool by eigen_schedule."""
    pool = eigen_pool(dim)
    kind, ent = eigen_schedule(npairs, stride)
    counts = np.zeros((npairs, dim * dim), np.int32); gaps = np.zeros(npairs, np.uint32); seqlen = np.zeros(npairs)
    for k, name in enumerate(EIGEN_KINDS):
        c, g, l = pool[name]
        sel = kind == k
        ix = ent[sel] % len(g)
        counts[sel], gaps[sel], seqlen[sel] = c[ix], g[ix], l[ix]
    return counts, gaps, seqlen, kind
