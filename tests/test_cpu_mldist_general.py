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
