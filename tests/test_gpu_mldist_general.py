"""pgm_mldist_general_kernel: ML distances for a general generator Q (no eigen form, dim <= 64) through pgm_mldist_batch.

The independent statement is tests/mldist_general_ref.py: the same Newton iteration with P(d) from the same scale / 20-term Taylor /
squaring recipe, in numpy float64.  Second witness where a model has both forms: a random reversible 20-state model, the kernel
given Q alone against the oracle's pgmo_mldist given the eigen form.

Models: random generators (rows summing to zero, positive off-diagonals, not reversible) of 4, 21 (the first dim beyond the eigen
kernel's limit), 61 and 64 (the maximum) states, and the shipped ECM codon model.  257 pairs per model (a grid tail; launches of
1, 5 and 257 pairs), twice: with the driver's default codon clamps and -m, and with clamps that reach the codon DIST_MAX of 5.2 and -M.
The pairs reach every branch (asserted on the statement's record of each pair): an identical pair, an empty pair, a p-distance
above 0.85, the MAXITER exit with and without an upper bracket, the gap term with non-zero gaps, a distance small enough for no
squaring, a distance of 5.2 with six.  Every pair is compared.

BOUND: ten times the largest relative difference between the kernel's arithmetic and the statement over all these cases, 5.7e-14
for the distances and 4.3e-13 for the variances (both on the 4-state generator, where f cancels most; 61 and 64 states and ECM:
4.3e-15 / 6.2e-14; the second witness: 4.4e-14 / 6.6e-14).  These figures are of the kernel's operations restated on the CPU in
their own order (products with k ascending, one multiply and one add per term, sums in storage order, glibc's log), which is the
host estimator's order; the kernel itself differs from that by the device library's log of the start value, and its own difference
on an MI355X, which every case prints before the assertion, is unmeasured."""
import ctypes as C

import numpy as np
import pytest

import mldist_general_ref as R

pytestmark = pytest.mark.gpu

DIST_BOUND = 10 * 5.7e-14
VAR_BOUND = 10 * 4.3e-13

MODELS = {
    "rand4": lambda: R.random_generator(4, 4),
    "rand21": lambda: R.random_generator(21, 21),
    "rand61": lambda: R.random_generator(61, 61),
    "rand64": lambda: R.random_generator(64, 64),
    "ecm": lambda: R.shipped_model("ecm.qmat"),
}
SETS = {"default_m": (R.CODON_PAR, 1, 0), "wide_M": (R.WIDE_PAR, 0, 1)}
_cache = {}


def _P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _model(Q, par, mldist, mldist_gap, eig=None):
    import prographmsa_amd as pg
    m = pg.pgm_mldist_model()
    keep = [np.asfortranarray(Q)]
    m.dim = Q.shape[0]
    m.Q = _P(keep[0], C.c_double)
    if eig is not None:
        keep += [np.asfortranarray(eig[0]), np.asfortranarray(eig[1]), np.ascontiguousarray(eig[2])]
        m.V, m.Vi, m.sigma = _P(keep[1], C.c_double), _P(keep[2], C.c_double), _P(keep[3], C.c_double)
    for k, v in par.items():
        setattr(m, k, v)
    m.mldist, m.mldist_gap = mldist, mldist_gap
    return m, keep


def _run(ctx, m, counts, gaps, seqlen, npairs):
    import prographmsa_amd as pg
    c = np.ascontiguousarray(counts[:npairs].reshape(-1)); g = np.ascontiguousarray(gaps[:npairs]); l = np.ascontiguousarray(seqlen[:npairs])
    dist = np.full(npairs, -7.0); var = np.full(npairs, -7.0)
    rc = pg.lib.pgm_mldist_batch(ctx.handle, C.byref(m), npairs, _P(c, C.c_int32), _P(g, C.c_uint32), _P(l, C.c_double), _P(dist, C.c_double), _P(var, C.c_double))
    return rc, dist, var


def _case(model, pset):
    """Model, pairs and the statement's result, computed once per (model, parameter set)."""
    if (model, pset) not in _cache:
        Q = MODELS[model]()
        counts, gaps, seqlen = R.kernel_test_pairs(Q, 5)
        par, ml, mg = SETS[pset]
        _cache[(model, pset)] = (Q, counts, gaps, seqlen) + R.estimate_batch(Q, counts, gaps, seqlen, par, ml, mg)
    return _cache[(model, pset)]


@pytest.mark.parametrize("pset", list(SETS))
@pytest.mark.parametrize("model", list(MODELS))
def test_general_kernel_against_the_numpy_statement(ctx, model, pset):
    import prographmsa_amd as pg
    Q, counts, gaps, seqlen, rd, rv, info = _case(model, pset)
    par, ml, mg = SETS[pset]
    # the inputs reach the branches (the statement's record)
    exits = {i["exit"] for i in info}
    sq = {s for i in info for s in i["squarings"]}
    assert info[1]["exit"] == "none" and info[1]["newton"] == 0 and counts[1].sum() > 0       # identical pair: no Newton
    assert info[2]["exit"] == "none" and counts[2].sum() == 0                                    # empty pair
    assert info[3]["start"] == "dist_max" and counts[3].sum() > 0                                # p-distance > 0.85
    assert "converged" in exits and "maxiter_unbracketed" in exits and 0 in sq
    if pset == "default_m":
        assert "maxiter_bracketed" in exits
    else:
        assert max(sq) >= 5 and gaps[0] > 0 and info[0]["exit"] == "converged"                   # 5.2 |Q|_1 > 16; the gap term on a converging pair
    m, keep = _model(Q, par, ml, mg)
    worst_d = worst_v = 0.0
    for npairs in (1, 5, R.NPAIRS):
        rc, dist, var = _run(ctx, m, counts, gaps, seqlen, npairs)
        assert rc == pg.PGM_OK, pg.lib.pgm_last_error()
        wd, wv = R.rel_diff(dist, rd[:npairs]), R.rel_diff(var, rv[:npairs])
        print("mldist general %s %s npairs %d: max rel diff dist %.3e var %.3e" % (model, pset, npairs, wd, wv))
        worst_d, worst_v = max(worst_d, wd), max(worst_v, wv)
    assert pg.lib.pgm_dist_last_kernel_ms(ctx.handle) > 0
    assert worst_d <= DIST_BOUND and worst_v <= VAR_BOUND, (worst_d, worst_v)


def test_general_form_against_the_oracle_eigen_form(ctx):
    """A random reversible 20-state model: the kernel given Q alone, the oracle's pgmo_mldist given V, V^-1 and sigma."""
    import oracle_lib
    import prographmsa_amd as pg
    rng = np.random.default_rng(78)
    D = 20
    pi = rng.dirichlet(np.ones(D) * 5)
    S = rng.gamma(0.5, 1.0, (D, D)); S = (S + S.T) / 2; np.fill_diagonal(S, 0)
    Q = S * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(1))
    Q /= -(pi * np.diag(Q)).sum()
    sig, V = np.linalg.eig(Q)
    sig, V = sig.real, V.real
    Vi = np.linalg.inv(V)
    counts, gaps, seqlen = R.kernel_test_pairs(Q, 6)
    worst_d = worst_v = 0.0
    for par, ml, mg in ((R.AA_PAR, 1, 0), (R.AA_PAR, 0, 1)):
        mg_, keep = _model(Q, par, ml, mg)
        me, keep2 = _model(Q, par, ml, mg, eig=(V, Vi, sig))
        rc, dist, var = _run(ctx, mg_, counts, gaps, seqlen, R.NPAIRS)
        assert rc == pg.PGM_OK, pg.lib.pgm_last_error()
        rd, rv = oracle_lib.mldist(me, counts.reshape(-1), gaps, seqlen)
        wd, wv = R.rel_diff(dist, rd), R.rel_diff(var, rv)
        print("mldist general vs oracle eigen form (-m %d -M %d): max rel diff dist %.3e var %.3e" % (ml, mg, wd, wv))
        worst_d, worst_v = max(worst_d, wd), max(worst_v, wv)
    assert worst_d <= DIST_BOUND and worst_v <= VAR_BOUND, (worst_d, worst_v)


def test_model_forms_the_abi_accepts(ctx):
    """dim = 61 with Q alone is accepted (PGM_ERR_INVALID before the general kernel); dim = 65, dim = 61 with an eigen form and a
    model with only some of V, Vi, sigma stay invalid; the eigen form with dim = 20 still runs."""
    import prographmsa_amd as pg
    rng = np.random.default_rng(3)

    def call(n, eig, partial=False):
        Q = R.random_generator(n, n)
        counts = np.ascontiguousarray(R.counts_at(Q, 0.3, 100, rng).reshape(1, -1, order="F").astype(np.int32))
        e = (np.eye(n), np.eye(n), np.zeros(n)) if eig else None
        m, keep = _model(Q, R.CODON_PAR, 1, 0, eig=e)
        if partial:
            m.Vi = None
        return _run(ctx, m, counts, np.array([1], np.uint32), np.array([100.0]), 1)

    rc, dist, var = call(61, False)
    assert rc == pg.PGM_OK and 0 < dist[0] <= 5.0 and var[0] > 0
    assert call(65, False)[0] == pg.PGM_ERR_INVALID
    assert call(61, True)[0] == pg.PGM_ERR_INVALID
    assert call(20, True, partial=True)[0] == pg.PGM_ERR_INVALID
    assert call(20, True)[0] == pg.PGM_OK
