"""Pins the numpy statement of the general-form ML distance estimator (tests/mldist_general_ref.py) against the host estimator,
without a GPU: the oracle driver's `--codon -a -m -T -i 0 --dump_dist` on a 12 x 60 codon family against the statement applied to
the pair counts of the oracle's alignPair (pgmo_nw_pairs_batch) and the ECM generator rebuilt from host/data/ecm.qmat.

BOUND 1e-9 (relative, distances and variances).  Both sides evaluate the same formulas in float64; they differ in the association
of the matrix products and sums (BLAS against the host's loops) and in the last bits of Q (numpy's solve against the host's
elimination for the frequencies that scale it).  An entry of exp(Q d / 2^s) carries a few dim * 2^-53 = 7e-15 of relative rounding
error, every one of the s <= 6 squarings at d <= 5 doubles it (4e-13), and the root of f = sum c P'/P moves by that error times
the cancellation in f, sum |c P'/P| / (d |f'|), below 1e3 for these counts: 4e-10, rounded up to the next power of ten."""
import os
import subprocess

import numpy as np
import pytest

import gen
import mldist_general_ref as R

BOUND = 1e-9


def codon_family_pairs(seqs):
    """Symbols (index among the 61 sense codons in TCAG order; a leading ATG is stripped as the driver strips it), offsets and the
    pairs i < j in the order of the dumped matrix (names sorted)."""
    syms, offs = [], [0]
    for s in seqs:
        cod = [s[k:k + 3] for k in range(0, len(s), 3)]
        if cod and cod[0] == "ATG":
            cod = cod[1:]
        syms += [gen.CODONS.index(c) for c in cod]
        offs.append(len(syms))
    n = len(seqs)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return np.array(syms, np.int8), np.array(offs, np.uint32), pairs


def statement_matrices(seqs):
    import oracle_lib
    syms, offs, pairs = codon_family_pairs(seqs)
    tok = open(os.path.join(R.DATA, "nw_codon.imat")).read().split()
    assert tok[0] == "62" and tok[1] == "62"
    score = np.array([int(x) for x in tok[2:2 + 62 * 62]], np.int32)
    counts, gaps = oracle_lib.nw_pairs(61, score, -10, -2, syms, offs, [p[0] for p in pairs], [p[1] for p in pairs])
    lens = np.diff(offs.astype(np.int64))
    seqlen = np.array([(lens[i] + lens[j]) / 2.0 for i, j in pairs])
    d, v, info = R.estimate_batch(R.shipped_model("ecm.qmat"), counts, gaps, seqlen, R.CODON_PAR, 1, 0)
    n = len(seqs)
    D, V = np.zeros((n, n)), np.zeros((n, n))
    for (i, j), dd, vv in zip(pairs, d, v):
        D[i, j] = D[j, i] = dd
        V[i, j] = V[j, i] = vv
    return D, V, info


def test_numpy_statement_matches_the_host_estimator(oracle_build, tmp_path):
    seqs = gen.gen_codon(12, 60, 41, sub=0.15)
    fa = tmp_path / "cod.fa"
    fa.write_text(gen.fasta(seqs))
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    dumps = []
    for device in (0, 1):      # (the oracle backend has no general-form estimator: with the switch set the host estimator still runs)
        env = dict(os.environ)
        env.pop("PGM_DEVICE_MLDIST", None)
        if device:
            env["PGM_DEVICE_MLDIST"] = "1"
        dump = tmp_path / ("dist%d.bin" % device)
        r = subprocess.run([exe, "--codon", "-a", "-m", "-T", "-i", "0", "--dump_dist", str(dump), str(fa)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        dumps.append(R.read_dump(str(dump)))
    (dh, vh), = dumps[0]
    assert np.array_equal(dh, dumps[1][0][0]) and np.array_equal(vh, dumps[1][0][1])
    D, V, info = statement_matrices(seqs)
    assert any(i["exit"] == "converged" for i in info)
    off = ~np.eye(12, dtype=bool)
    wd = R.rel_diff(D[off], dh.reshape(12, 12)[off])
    wv = R.rel_diff(V[off], vh.reshape(12, 12)[off])
    print("numpy statement vs host estimator: max rel diff dist %.3e var %.3e (%d of 66 pairs converged)" % (wd, wv, sum(i["exit"] == "converged" for i in info)))
    assert wd <= BOUND and wv <= BOUND, (wd, wv)


# ---- the CPU companion of tests/test_gpu_dist.py::test_mldist_eigen_kernel_dims_and_grid_rounds --------------------------------
# The GPU test compares the eigen-form kernel with the oracle's pgmo_mldist to 1e-12 (distances) and 1e-9 (variances) on pairs it
# draws from R.eigen_pool.  Two independent evaluations of the estimator may legitimately part where a pair sits on one of its
# branch edges (the MAXITER exit, the 0.85 switch of the start value, the final clamps).  That no pool entry does is checked here
# with a second witness: the oracle given the eigen form against the numpy statement given Q alone (P(d) by Taylor series and
# squarings instead of V exp(sigma d) V^-1), to a tenth of the GPU test's tolerances.  Every entry of the pool is compared.
EIGEN_DIST_BOUND = 1e-12 / 10
EIGEN_VAR_BOUND = 1e-9 / 10


@pytest.mark.parametrize("flags", R.EIGEN_FLAGS)
@pytest.mark.parametrize("dim", R.EIGEN_DIMS)
def test_eigen_pool_sits_on_no_branch_edge(oracle_build, dim, flags):
    import oracle_lib
    Q = R.eigen_model(dim)[0]
    m, keep = R.eigen_ctypes_model(dim, flags)
    pool = R.eigen_pool(dim)
    worst_d = worst_v = 0.0
    for kind in R.EIGEN_KINDS:
        counts, gaps, seqlen = pool[kind]
        od, ov = oracle_lib.mldist(m, counts.reshape(-1), gaps, seqlen)
        sd, sv, info = R.estimate_batch(Q, counts, gaps, seqlen, R.AA_PAR, *flags)
        # the kinds are what their names say (the statement's record of each pair)
        tot = counts.sum(1)
        if kind == "near":
            assert all(i["start"] == "pdist" and i["newton"] > 0 for i in info)
        elif kind == "far":      # (at 19 and 20 states a pair at distance 3 has a p-distance above 0.85 and starts at DIST_MAX)
            assert all(i["newton"] > 0 for i in info)
        elif kind == "empty":
            assert not tot.any() and all(i["newton"] == 0 for i in info)
        elif kind == "identical":
            assert tot.all() and all(i["start"] == "pdist" and i["newton"] == 0 for i in info)
        else:
            assert all(i["start"] == "dist_max" and i["newton"] > 0 for i in info)
        wd, wv = R.rel_diff(sd, od), R.rel_diff(sv, ov)
        print("eigen pool dim %d -m %d -M %d %-9s: %d pairs, oracle eigen form vs numpy statement max rel diff dist %.3e var %.3e" % (dim, flags[0], flags[1], kind, len(gaps), wd, wv))
        worst_d, worst_v = max(worst_d, wd), max(worst_v, wv)
    assert worst_d <= EIGEN_DIST_BOUND and worst_v <= EIGEN_VAR_BOUND, (worst_d, worst_v)


def test_eigen_schedule_changes_kind_between_rounds():
    """Pairs p and p + stride (one wavefront, consecutive rounds of the grid) are of different kinds, every kind and every pool entry
    is used, for the strides of 4 .. 304 CUs (stride = 4 wavefronts x 2 blocks per CU)."""
    for cus in (1, 4, 80, 104, 256, 304):
        stride = 8 * cus
        npairs = int(2.5 * stride) + 3
        kind, ent = R.eigen_schedule(npairs, stride)
        assert np.all(kind[:-stride] != kind[stride:])
        assert set(kind.tolist()) == set(range(len(R.EIGEN_KINDS)))
    counts, gaps, seqlen, kind = R.eigen_pairs(4, int(2.5 * 2048), 2048)
    pool = R.eigen_pool(4)
    for k, name in enumerate(R.EIGEN_KINDS):
        got = {c.tobytes() for c in counts[kind == k]}
        assert got == {c.tobytes() for c in pool[name][0]}
