"""GPU parity for the two satellite stages through the C ABI: all-pairs NW counts (bit-exact int32) and
context-specific profiles (fp64, tolerance 1e-12 relative: only the device exp() differs from glibc)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _nw_gpu(ctx, dim, score, go, ge, syms, offs, pi, pj):
    import prographmsa_amd as pg
    score = np.ascontiguousarray(score, np.int32); syms = np.ascontiguousarray(syms, np.int8)
    offs = np.ascontiguousarray(offs, np.uint32); pi = np.ascontiguousarray(pi, np.uint32); pj = np.ascontiguousarray(pj, np.uint32)
    npairs = len(pi)
    counts = np.full(max(1, npairs * dim * dim), -1, np.int32)
    gaps = np.zeros(max(1, npairs), np.uint32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    pg.check(pg.lib.pgm_nw_pairs_batch(ctx.handle, dim, P(score, C.c_int32), go, ge, len(offs) - 1, P(syms, C.c_int8), P(offs, C.c_uint32),
                                       npairs, P(pi, C.c_uint32), P(pj, C.c_uint32), P(counts, C.c_int32), P(gaps, C.c_uint32)))
    return counts[: npairs * dim * dim].reshape(npairs, dim * dim), gaps[:npairs]


def _nw_submit(ctx, dim, score, go, ge, syms, offs, pi, pj, flags=0):
    """pgm_nw_pairs_submit + pgm_nw_pairs_wait.  Returns (rc of the submit or of the wait, counts, gaps); counts has 2 entries per
    pair with PGM_NW_REDUCED, dim * dim without."""
    import prographmsa_amd as pg
    score = np.ascontiguousarray(score, np.int32); syms = np.ascontiguousarray(syms, np.int8)
    offs = np.ascontiguousarray(offs, np.uint32); pi = np.ascontiguousarray(pi, np.uint32); pj = np.ascontiguousarray(pj, np.uint32)
    npairs = len(pi)
    per = 2 if flags & pg.PGM_NW_REDUCED else dim * dim
    counts = np.full(max(1, npairs * per), -1, np.int32)
    gaps = np.zeros(max(1, npairs), np.uint32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    t = C.c_int(-1)
    rc = pg.lib.pgm_nw_pairs_submit(ctx.handle, dim, P(score, C.c_int32), go, ge, len(offs) - 1, P(syms, C.c_int8), P(offs, C.c_uint32), npairs,
                                    P(pi, C.c_uint32), P(pj, C.c_uint32), flags, P(counts, C.c_int32), P(gaps, C.c_uint32), C.byref(t))
    if rc == pg.PGM_OK:
        rc = pg.lib.pgm_nw_pairs_wait(ctx.handle, t.value)
    return rc, counts[: npairs * per].reshape(npairs, per), gaps[:npairs]


def _related(rng, dim, lens, base, exact=False):
    """Sequences cut from one base sequence, each with 20 % of its symbols redrawn from 0 .. dim (dim: the symbol that is not counted)
    and, beyond 10 symbols, one deletion of 1 .. 4: related, so that the traceback has matches, mismatches and gaps.  exact: the
    sequences have exactly the lengths asked for (otherwise a deletion shortens them)."""
    seqs = []
    for L in lens:
        k = int(rng.integers(1, 5)) if exact and L > 10 else 0
        s = base[:L + k].copy()
        mut = rng.random(L + k) < 0.2
        s[mut] = rng.integers(0, dim + 1, mut.sum())   # dim == the "invalid -> 20" style extra symbol when dim == 20
        if exact and k:
            cut = int(rng.integers(1, L - 5))
            s = np.concatenate([s[:cut], s[cut + k:]])
        elif L > 10:
            cut = int(rng.integers(1, L - 5))
            s = np.concatenate([s[:cut], s[cut + int(rng.integers(1, 5)):]])
        seqs.append(np.minimum(s, dim).astype(np.int8))
    return seqs


def _pack(seqs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    syms = np.concatenate(seqs) if len(seqs) else np.zeros(0, np.int8)
    return syms, offs


def _score(dim, rng):
    s = rng.integers(-4, 3, (dim + 1, dim + 1)).astype(np.int32)
    s = np.minimum(s, s.T)
    s[np.arange(dim + 1), np.arange(dim + 1)] = rng.integers(4, 12, dim + 1)
    return s.reshape(-1)


@pytest.mark.parametrize("dim", [1, 4, 20, 21, 33, 61])
def test_nw_pairs_bit_exact(ctx, dim):
    import oracle_lib
    rng = np.random.default_rng(5 + dim)
    # the kernel sweeps bands of 512 rows (8 rows per lane) and stores 2 steps per direction word: lengths around those edges
    lens = [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 333, 511, 512, 513, 700, 1030]
    seqs = _related(rng, dim, lens, rng.integers(0, dim, 1100))
    syms, offs = _pack(seqs)
    pi, pj = zip(*[(i, j) for i in range(len(seqs)) for j in range(len(seqs)) if i != j])
    score = _score(dim, rng)
    cg, gg = _nw_gpu(ctx, dim, score, -10, -2, syms, offs, pi, pj)
    co, go_ = oracle_lib.nw_pairs(dim, score, -10, -2, syms, offs, pi, pj)
    assert np.array_equal(cg, co)
    assert np.array_equal(gg, go_)


def test_nw_two_tiles_in_flight_reduced_and_pinned(ctx):
    """pgm_nw_pairs_submit / _wait: two tiles in flight on one context (pageable and pinned result buffers), a third submit is
    refused, PGM_NW_REDUCED returns (trace, sum) of the count matrices; all against the oracle's full matrices."""
    import oracle_lib
    import prographmsa_amd as pg
    rng = np.random.default_rng(77)
    dim = 20
    base = rng.integers(0, dim, 700)
    seqs = []
    for L in [40, 300, 511, 513, 640, 700, 90, 257, 129, 64]:
        s_ = base[:L].copy()
        mut = rng.random(L) < 0.25
        s_[mut] = rng.integers(0, dim + 1, mut.sum())
        seqs.append(np.minimum(s_, dim).astype(np.int8))
    offs = np.concatenate([[0], np.cumsum([len(s_) for s_ in seqs])]).astype(np.uint32)
    syms = np.concatenate(seqs)
    pairs = [(i, j) for i in range(len(seqs)) for j in range(i + 1, len(seqs))]
    score = np.ascontiguousarray(_score(dim, rng), np.int32)
    co, go_ = oracle_lib.nw_pairs(dim, score, -10, -2, syms, offs, [a for a, _ in pairs], [b for _, b in pairs])
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    half = len(pairs) // 2
    tiles = [pairs[:half], pairs[half:]]
    for flags, per in ((0, dim * dim), (pg.PGM_NW_REDUCED, 2)):
        for pinned in (False, True):
            bufs, tickets, keep = [], [], []
            for tl in tiles:
                pi = np.array([a for a, _ in tl], np.uint32); pj = np.array([b for _, b in tl], np.uint32)
                if pinned:
                    cp, gp = pg.lib.pgm_host_alloc(len(tl) * per * 4), pg.lib.pgm_host_alloc(len(tl) * 4)
                    assert cp and gp
                    c = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_int32)), (len(tl) * per,)); g = np.ctypeslib.as_array(C.cast(gp, C.POINTER(C.c_uint32)), (len(tl),))
                    keep.append((cp, gp))
                else:
                    c, g = np.full(len(tl) * per, -7, np.int32), np.zeros(len(tl), np.uint32)
                t = C.c_int(-1)
                pg.check(pg.lib.pgm_nw_pairs_submit(ctx.handle, dim, P(score, C.c_int32), -10, -2, len(seqs), P(syms, C.c_int8), P(offs, C.c_uint32), len(tl),
                                                    P(pi, C.c_uint32), P(pj, C.c_uint32), flags, P(c, C.c_int32), P(g, C.c_uint32), C.byref(t)))
                bufs.append((c, g, pi, pj)); tickets.append(t.value)
            assert sorted(tickets) == [0, 1]
            t = C.c_int(-1)
            c3, g3 = np.zeros(per, np.int32), np.zeros(1, np.uint32)
            rc = pg.lib.pgm_nw_pairs_submit(ctx.handle, dim, P(score, C.c_int32), -10, -2, len(seqs), P(syms, C.c_int8), P(offs, C.c_uint32), 1,
                                            P(bufs[0][2], C.c_uint32), P(bufs[0][3], C.c_uint32), flags, P(c3, C.c_int32), P(g3, C.c_uint32), C.byref(t))
            assert rc == pg.PGM_ERR_INVALID                       # a third tile without a wait
            for k in (0, 1):
                pg.check(pg.lib.pgm_nw_pairs_wait(ctx.handle, tickets[k]))
            assert pg.lib.pgm_nw_pairs_wait(ctx.handle, 0) == pg.PGM_ERR_INVALID   # nothing in flight any more
            got_c = np.concatenate([b[0] for b in bufs]).reshape(len(pairs), per)
            got_g = np.concatenate([b[1] for b in bufs])
            assert np.array_equal(got_g, go_)
            if flags:
                cm = co.reshape(len(pairs), dim, dim)
                assert np.array_equal(got_c[:, 0], np.trace(cm, axis1=1, axis2=2)) and np.array_equal(got_c[:, 1], cm.sum((1, 2)))
            else:
                assert np.array_equal(got_c, co)
            del bufs, got_c, got_g
            for cp, gp in keep:
                pg.lib.pgm_host_free(cp); pg.lib.pgm_host_free(gp)


def test_nw_empty(ctx):
    c, g = _nw_gpu(ctx, 20, _score(20, np.random.default_rng(0)), -10, -2, np.zeros(4, np.int8), [0, 4], [], [])
    assert c.size == 0 and g.size == 0


_reuse = {}


def _reuse_case(cus):
    """Sequences, pairs and the oracle's result of test_nw_queue_reuse_bit_exact, computed once for its four parametrisations."""
    if cus not in _reuse:
        import oracle_lib
        rng = np.random.default_rng(2024)
        dim = 4
        slots_max = cus * 8 * 4                                   # blocks <= cus x min(per_cu, 8), 4 wavefronts each
        n = int(np.ceil(np.sqrt(4 * slots_max)))                  # n x n ordered pairs >= 4 x the slots
        lens = [0, 1, 63, 64, 65, 127, 128, 129] + rng.integers(0, 131, n - 8).tolist()
        seqs = _related(rng, dim, lens, rng.integers(0, dim, 140), exact=True)
        assert [len(q) for q in seqs] == lens
        syms, offs = _pack(seqs)
        assert (syms == dim).any()                                # the symbol that is not counted
        pairs = [(i, j) for i in range(n) for j in range(n)]      # all ordered pairs, (i, i) among them
        pairs += [pairs[k] for k in rng.integers(0, len(pairs), 300)]   # and repeated ones
        pi = np.array([a for a, _ in pairs], np.uint32); pj = np.array([b for _, b in pairs], np.uint32)
        score = _score(dim, rng)
        co, go_ = oracle_lib.nw_pairs(dim, score, -10, -2, syms, offs, pi, pj)
        cost = np.array(lens, np.int64)[pi] * np.array(lens, np.int64)[pj]
        _reuse[cus] = dict(dim=dim, syms=syms, offs=offs, pi=pi, pj=pj, score=score, counts=co, gaps=go_, cost=cost,
                           shuffle=rng.permutation(len(pairs)))
        for a in _reuse[cus].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _reuse[cus]


@pytest.mark.parametrize("reduced", [False, True])
@pytest.mark.parametrize("presorted", [False, True])
def test_nw_queue_reuse_bit_exact(ctx, presorted, reduced):
    """The persistent grid with more than four pairs per wavefront slot: a slot's direction words are laid out anew for every pair
    (twords changes), its brow row and the registers of the band loop carry the previous pair's values.  dim 4 with the uncounted
    symbol 4, lengths 0 .. 130 (no band edge: what is under test is the loop around the pair, not the pair), all ordered pairs
    with (i, i) and 300 repeated ones; shuffled (the order pass sorts) or handed over longest first (the order pass finds them
    sorted and keeps the identity); full count matrices or PGM_NW_REDUCED.  Every pair against the oracle."""
    import prographmsa_amd as pg
    cus = ctx.device_info()[1]
    c = _reuse_case(cus)
    npairs = len(c["pi"])
    assert npairs > cus * 8 * 4 and npairs >= 4 * cus * 8 * 4      # more pairs than the launch can have slots: slots are reused
    perm = np.argsort(-c["cost"], kind="stable") if presorted else c["shuffle"]
    cost = c["cost"][perm]
    assert bool(np.all(cost[1:] <= cost[:-1])) == presorted
    dim = c["dim"]
    rc, cg, gg = _nw_submit(ctx, dim, c["score"], -10, -2, c["syms"], c["offs"], c["pi"][perm], c["pj"][perm], pg.PGM_NW_REDUCED if reduced else 0)
    assert rc == pg.PGM_OK
    co, go_ = c["counts"][perm], c["gaps"][perm]
    assert np.array_equal(gg, go_)
    if reduced:
        cm = co.reshape(npairs, dim, dim)
        assert np.array_equal(cg[:, 0], np.trace(cm, axis1=1, axis2=2)) and np.array_equal(cg[:, 1], cm.sum((1, 2)))
    else:
        assert np.array_equal(cg, co)


GAP_SETTINGS = [(-10, -2), (-3, -3), (0, 0), (-2, -7), (-40, -25)]
SCORE_KINDS = ["random_asym", "zero", "match1", "large_asym"]
PARAM_LENS = [0, 1, 2, 8, 9, 63, 64, 65, 400, 401, 511, 512, 513, 530]
_param_seqs = {}


def _param_case(dim):
    """The 14 mutually related sequences of PARAM_LENS and two unrelated ones (300 and 77 symbols), all 256 ordered pairs."""
    if dim not in _param_seqs:
        rng = np.random.default_rng(600 + dim)
        seqs = _related(rng, dim, PARAM_LENS, rng.integers(0, dim, 540), exact=True)
        seqs += [rng.integers(0, dim + 1, 300).astype(np.int8), rng.integers(0, dim + 1, 77).astype(np.int8)]
        assert [len(q) for q in seqs[:len(PARAM_LENS)]] == PARAM_LENS
        syms, offs = _pack(seqs)
        n = len(seqs)
        pi = np.repeat(np.arange(n), n).astype(np.uint32); pj = np.tile(np.arange(n), n).astype(np.uint32)
        _param_seqs[dim] = (seqs, syms, offs, pi, pj)
    return _param_seqs[dim]


def _gotoh_W(score, sd, go, ge, s1, s2):
    """W of the plain recurrence (DistanceFactoryAlign.h:59-91; rows: s2, columns: s1), for the statements about the values it reaches."""
    MINF = -10000
    s1, s2 = [int(v) for v in s1], [int(v) for v in s2]
    W = np.zeros((len(s2) + 1, len(s1) + 1), np.int64); X = W.copy(); Y = W.copy()
    W[0, 1:] = X[0, 1:] = go + np.arange(len(s1)) * ge; Y[0, 1:] = MINF
    W[1:, 0] = Y[1:, 0] = go + np.arange(len(s2)) * ge; X[1:, 0] = MINF
    for y in range(1, len(s2) + 1):
        for x in range(1, len(s1) + 1):
            X[y, x] = max(X[y, x - 1] + ge, W[y, x - 1] + go)
            Y[y, x] = max(Y[y - 1, x] + ge, W[y - 1, x] + go)
            W[y, x] = max(W[y - 1, x - 1] + score[s2[y - 1] + sd * s1[x - 1]], X[y, x], Y[y, x])
    return W


@pytest.mark.parametrize("dim", [4, 20])
@pytest.mark.parametrize("kind", SCORE_KINDS)
@pytest.mark.parametrize("gap", GAP_SETTINGS, ids=lambda g: "go%d_ge%d" % g)
def test_nw_scoring_parameters_bit_exact(ctx, gap, kind, dim):
    """Scores and gap penalties beyond the one setting of the tests above, against the oracle, bit for bit.
    random_asym / large_asym: score != score.T, so a transposed look-up (score[s1 + sd s2] for score[s2 + sd s1]) or a transposed
    count shows.  zero: every cell is a three-way tie, match1: most are: the priority diag >= max(X, Y), then X >= Y decides every
    step of the traceback.  (-3, -3), (0, 0), (-2, -7): opening equal to, free like, cheaper than extension.
    (-40, -25): the reference's minfty = -10000 is a finite number, and with these penalties the border W(y, 0) = go + (y - 1) ge
    lies below X(y, 0) = minfty from row 400 on: in the first band of 512 rows and, through brow, in the second; the kernel's
    folded constants (Wg = W + go, Xe = X + ge, MINF + ge) must still give the plain recurrence's values there.  Interior cells
    then fall below minfty as well (asserted on the recurrence itself, on the pair of 9 columns x 513 rows); with the other four
    settings no cell can, whatever the scores: W(y, x) >= 2 go + (x + y - 2) ge >= -7410 at these lengths."""
    import oracle_lib
    go, ge = gap
    seqs, syms, offs, pi, pj = _param_case(dim)
    sd = dim + 1
    rng = np.random.default_rng(31 * dim + 7 * SCORE_KINDS.index(kind))
    if kind == "random_asym":
        score = rng.integers(-6, 13, (sd, sd)).astype(np.int32)
    elif kind == "zero":
        score = np.zeros((sd, sd), np.int32)
    elif kind == "match1":
        score = np.eye(sd, dtype=np.int32)
    else:
        score = rng.integers(-3000, 3001, (sd, sd)).astype(np.int32)
    if kind.endswith("asym"):
        assert not np.array_equal(score, score.T)
    score = np.ascontiguousarray(score.reshape(-1))
    if gap == (-40, -25):
        assert go + (max(PARAM_LENS) - 1) * ge < -10000
        below = [y for y in range(1, max(PARAM_LENS) + 1) if go + (y - 1) * ge < -10000]     # rows whose border is below minfty
        assert below[0] <= 512 < below[-1]                                                   # in the first band and in a later one
        assert any(below[0] <= L <= 512 for L in PARAM_LENS) and any(L > 512 for L in PARAM_LENS)
        W = _gotoh_W(score, sd, go, ge, seqs[PARAM_LENS.index(9)], seqs[PARAM_LENS.index(513)])
        assert (W[1:, 1:] < -10000).any()
    cg, gg = _nw_gpu(ctx, dim, score, go, ge, syms, offs, pi, pj)
    co, go_ = oracle_lib.nw_pairs(dim, score, go, ge, syms, offs, pi, pj)     # (asserts PGM_OK: no backtracking error on any pair)
    assert np.array_equal(cg, co)
    assert np.array_equal(gg, go_)


def test_nw_rejects_bad_input(ctx):
    """The argument checks of pgm_nw_pairs_submit: PGM_ERR_INVALID for dim 0 and 62, a symbol of dim + 1, a negative symbol, a pair
    index == nseq and an unknown flag; dim 61 (the maximum) runs; the context still works after the refusals."""
    import oracle_lib
    import prographmsa_amd as pg
    rng = np.random.default_rng(9)

    def case(dim):
        seqs = _related(rng, dim, [0, 1, 30, 65, 130], rng.integers(0, dim, 140), exact=True)
        syms, offs = _pack(seqs)
        n = len(seqs)
        pi = np.repeat(np.arange(n), n).astype(np.uint32); pj = np.tile(np.arange(n), n).astype(np.uint32)
        return syms, offs, pi, pj, _score(dim, rng)

    syms, offs, pi, pj, score = case(20)
    big = _score(62, rng)
    assert _nw_submit(ctx, 0, big, -10, -2, syms, offs, pi, pj)[0] == pg.PGM_ERR_INVALID
    assert _nw_submit(ctx, 62, big, -10, -2, syms, offs, pi, pj)[0] == pg.PGM_ERR_INVALID
    bad = syms.copy(); bad[40] = 21
    assert _nw_submit(ctx, 20, score, -10, -2, bad, offs, pi, pj)[0] == pg.PGM_ERR_INVALID
    bad = syms.copy(); bad[40] = -1
    assert _nw_submit(ctx, 20, score, -10, -2, bad, offs, pi, pj)[0] == pg.PGM_ERR_INVALID
    bad = pi.copy(); bad[3] = len(offs) - 1
    assert _nw_submit(ctx, 20, score, -10, -2, syms, offs, bad, pj)[0] == pg.PGM_ERR_INVALID
    assert _nw_submit(ctx, 20, score, -10, -2, syms, offs, pi, bad)[0] == pg.PGM_ERR_INVALID
    assert _nw_submit(ctx, 20, score, -10, -2, syms, offs, pi, pj, flags=2)[0] == pg.PGM_ERR_INVALID
    # a valid call on the same context after the refusals, then the largest alphabet
    for dim, (sy, of, a, b, sc) in ((20, (syms, offs, pi, pj, score)), (61, case(61))):
        rc, cg, gg = _nw_submit(ctx, dim, sc, -10, -2, sy, of, a, b)
        assert rc == pg.PGM_OK
        co, go_ = oracle_lib.nw_pairs(dim, sc, -10, -2, sy, of, a, b)
        assert np.array_equal(cg, co) and np.array_equal(gg, go_)


def _cs_case(seed, K, ncols, lens, extra=()):
    """A random library of K context profiles of ncols columns (the loader's layout: log-probabilities times the column weights,
    a 21st entry of 0 for an invalid residue; the centre column's probabilities; log priors) and random sequences of the lengths
    `lens` (symbols 0 .. 20) followed by the sequences `extra`, with their tau, pi and uniform-prior profiles."""
    rng = np.random.default_rng(seed)
    p = rng.gamma(0.3, 1.0, (K, ncols, 20)) + 1e-4
    p /= p.sum(2, keepdims=True)
    w = 1.3 * 0.9 ** np.abs(np.arange(ncols) - ncols // 2)
    lp = np.zeros((K, ncols, 21))
    lp[:, :, :20] = np.log(p) * w[None, :, None]
    centre = p[:, ncols // 2, :].copy()
    priors = np.log(rng.dirichlet(np.ones(K)))
    seqs = [rng.integers(0, 21, L).astype(np.int8) for L in lens] + [np.asarray(e, np.int8) for e in extra]
    lens = [len(q) for q in seqs]
    c = dict(K=K, ncols=ncols, lens=lens, seqs=seqs)
    c["offs"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    c["syms"] = np.concatenate(seqs).astype(np.int8) if seqs else np.zeros(0, np.int8)
    c["out_offs"] = np.concatenate([[0], np.cumsum([20 * (L + 2) for L in lens])]).astype(np.uint64)
    c["tau"] = rng.uniform(0.05, 0.9, len(lens))
    c["pi"] = rng.dirichlet(np.ones(20) * 5)
    c["pu"] = rng.dirichlet(np.ones(20), len(lens))
    c["lpf"], c["cf"], c["prf"], c["puf"] = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (lp, centre, priors, c["pu"])]
    return c


def _cs_load(ctx, c, K=None, ncols=None):
    import prographmsa_amd as pg
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    return pg.lib.pgm_csprofile_load(ctx.handle, c["K"] if K is None else K, c["ncols"] if ncols is None else ncols,
                                     P(c["lpf"], C.c_double), P(c["cf"], C.c_double), P(c["prf"], C.c_double))


def _cs_create(ctx, c):
    import prographmsa_amd as pg
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    out = np.full(int(c["out_offs"][-1]), np.nan)
    pg.check(pg.lib.pgm_csprofile_create_batch(ctx.handle, len(c["lens"]), P(c["syms"], C.c_int8), P(c["offs"], C.c_uint32), P(c["tau"], C.c_double),
                                               P(c["pi"], C.c_double), P(c["puf"], C.c_double), P(out, C.c_double), P(c["out_offs"], C.c_uint64)))
    return out


def _cs_check(c, out):
    import oracle_lib
    for s in range(len(c["lens"])):
        ref = oracle_lib.csprofile_create(c["K"], c["ncols"], c["lpf"], c["cf"], c["prf"], c["seqs"][s], c["tau"][s], c["pi"], c["pu"][s])
        got = out[int(c["out_offs"][s]): int(c["out_offs"][s + 1])]
        assert np.all(np.isfinite(got))
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


CS_LENS = [0, 1, 5, 12, 13, 14, 100, 257]


def test_csprofile_matches_oracle(ctx):
    import prographmsa_amd as pg
    c = _cs_case(3, 37, 13, CS_LENS)
    pg.check(_cs_load(ctx, c))
    _cs_check(c, _cs_create(ctx, c))


@pytest.mark.parametrize("K,ncols", [(K, 13) for K in (1, 3, 4, 5, 6, 15, 16, 17, 33)] + [(17, n) for n in (1, 2, 12, 31)])
def test_csprofile_library_shapes(ctx, K, ncols):
    """The library streams through LDS in chunks of PGM_CS_KC = 16 profiles, evaluated PGM_CS_U = 4 at a time: K below one group
    (1, 3), one group and a tail of one or two (4, 5, 6), around a chunk (15, 16, 17), one past two chunks (33).  Window widths the ABI accepts
    besides 13: 1, even ones (2, 12: the columns are the offsets -ncols / 2 .. ncols / 2 - 1) and the maximum 31 (90 KB of LDS
    for a chunk).  Sequences around the window width and one of invalid residues only.  A width of 32 and K = 0 are refused, and
    the context still loads and creates after the refusals."""
    import prographmsa_amd as pg
    lens = CS_LENS + ([ncols - 1, ncols, ncols + 1] if ncols == 31 else [])
    c = _cs_case(1000 + 40 * K + ncols, K, ncols, lens, extra=[np.full(40, 20, np.int8)])
    wide = _cs_case(1, 1, 32, [])
    assert _cs_load(ctx, wide) == pg.PGM_ERR_INVALID
    assert _cs_load(ctx, c, K=0) == pg.PGM_ERR_INVALID
    pg.check(_cs_load(ctx, c))
    _cs_check(c, _cs_create(ctx, c))


def test_csprofile_small_library_after_a_large_one(ctx):
    """K = 33 and then K = 3 loaded on one context: the profiles of the smaller library see nothing of the larger one."""
    import prographmsa_amd as pg
    big, small = _cs_case(11, 33, 13, CS_LENS), _cs_case(12, 3, 13, CS_LENS)
    pg.check(_cs_load(ctx, big))
    _cs_check(big, _cs_create(ctx, big))
    pg.check(_cs_load(ctx, small))
    _cs_check(small, _cs_create(ctx, small))


def test_csprofile_profiles_left_on_the_device(ctx):
    """pgm_csprofile_create_batch_res (the leaf graphs of a resident pass with --cs_profile): the matrices stay in the context's
    resident arena.  Two such leaves aligned through pgm_site_ref give the score bits and mappings of the same two graphs with the
    host variant's columns uploaded the ordinary way — the kernel and its output are the same, only the destination differs."""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    c = _cs_case(5, 23, 13, [83, 140])
    lens, syms, offs, tau, pi, puf, out_offs = c["lens"], c["syms"], c["offs"], c["tau"], c["pi"], c["puf"], c["out_offs"]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    pg.check(_cs_load(ctx, c))
    out = _cs_create(ctx, c)
    dev = (C.POINTER(C.c_double) * 2)()
    pg.check(pg.lib.pgm_resident_reset(ctx.handle))
    pg.check(pg.lib.pgm_csprofile_create_batch_res(ctx.handle, 2, P(syms, C.c_int8), P(offs, C.c_uint32), P(tau, C.c_double),
                                                   P(pi, C.c_double), P(puf, C.c_double), dev))
    job = J.random_job(4343, lens[0] + 2, lens[1] + 2, dim=20, skip_frac=0.0, drop_chain_frac=0.0)
    job.g1.sites = out[int(out_offs[0]): int(out_offs[1])].copy()
    job.g2.sites = out[int(out_offs[1]): int(out_offs[2])].copy()
    b = J.Batch(ctx, [job])
    b.run()
    want = b.fetch()[0]
    b.close()
    cj = J.CJobs([job])
    r1 = (pg.pgm_site_ref * 1)(); r2 = (pg.pgm_site_ref * 1)()
    r1[0].dev_sites, r1[0].node_map, r1[0].ncols = dev[0], None, lens[0] + 2
    r2[0].dev_sites, r2[0].node_map, r2[0].ncols = dev[1], None, lens[1] + 2
    pg.check(pg.lib.pgm_align_graphs_batch_res(ctx.handle, 1, cj.g1, cj.g2, cj.m, cj.sc, r1, r2, cj.out))
    got = cj.results()[0]
    assert want["status"] == 0 and np.float32(got["score"]).view(np.uint32) == np.float32(want["score"]).view(np.uint32)
    assert np.array_equal(got["map1"], want["map1"]) and np.array_equal(got["map2"], want["map2"])


def test_csprofile_config5_scale_sample(ctx):
    """BASELINE config 5 scale: the synthetic K = 4000 library and 1024 leaves x 600 residues of bench.py's `csprofile` record
    (same generator, same seeds); every 64th leaf is compared with the oracle (the library streams through LDS in 250 chunks)."""
    import oracle_lib
    import prographmsa_amd as pg
    rng = np.random.default_rng(5)
    K, ncols, nleaf, L = 4000, 13, 1024, 600
    p = rng.gamma(0.3, 1.0, (K, ncols, 20)) + 1e-4
    p /= p.sum(2, keepdims=True)
    w = 1.3 * 0.9 ** np.abs(np.arange(ncols) - ncols // 2)
    lp = np.zeros((K, ncols, 21))
    lp[:, :, :20] = np.log(p) * w[None, :, None]
    lpf = np.ascontiguousarray(lp, np.float64).reshape(-1)
    cf = np.ascontiguousarray(p[:, ncols // 2, :], np.float64).reshape(-1)
    prf = np.log(rng.dirichlet(np.ones(K)))
    syms = rng.integers(0, 20, nleaf * L).astype(np.int8)
    offs = (np.arange(nleaf + 1) * L).astype(np.uint32)
    out_offs = (np.arange(nleaf + 1) * 20 * (L + 2)).astype(np.uint64)
    tau = np.full(nleaf, 0.3)
    pi = np.full(20, 0.05)
    pu = np.full(nleaf * 20, 0.05)
    out = np.full(int(out_offs[-1]), np.nan)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    pg.check(pg.lib.pgm_csprofile_load(ctx.handle, K, ncols, P(lpf, C.c_double), P(cf, C.c_double), P(prf, C.c_double)))
    pg.check(pg.lib.pgm_csprofile_create_batch(ctx.handle, nleaf, P(syms, C.c_int8), P(offs, C.c_uint32), P(tau, C.c_double),
                                               P(pi, C.c_double), P(pu, C.c_double), P(out, C.c_double), P(out_offs, C.c_uint64)))
    assert np.all(np.isfinite(out))
    for s in range(0, nleaf, 64):
        ref = oracle_lib.csprofile_create(K, ncols, lpf, cf, prf, syms[s * L:(s + 1) * L], 0.3, pi, pu[s * 20:(s + 1) * 20])
        np.testing.assert_allclose(out[int(out_offs[s]): int(out_offs[s + 1])], ref, rtol=1e-12, atol=0)
