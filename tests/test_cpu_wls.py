"""Weighted least-squares guide-tree refinement (-W / -WW; reference src/LeastSquares.cpp, src/NNLS.h) through the CPU
oracle driver, whose subtree pair sums are the host's statement of the kernels' order (Backend::wls_pair_sums_batch).

The driver's newicks and FASTA are compared with the reference binary's (tests/golden/wls.json, make_golden_wls.py), and the
NNLS restatement (prographmsa_amd/host/nnls.h) with a numpy statement of the reference's active-set loop."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

import sys  # noqa: E402
sys.path.insert(0, GOLD)
import make_golden_wls as MG  # noqa: E402

WLS = json.load(open(os.path.join(GOLD, "wls.json")))
KNOWN = json.load(open(os.path.join(GOLD, "wls_known_mismatch.json")))


def run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def write_family(tmp_path, rec):
    fa = tmp_path / "f.fa"
    fa.write_text(MG.family(rec["n"], rec["L"], rec["seed"], rec["sub"], rec["indel"], rec["dups"]))
    return str(fa)


@pytest.mark.parametrize("idx", range(len(WLS["trees"])), ids=lambda i: "n%d" % WLS["trees"][i]["n"])
@pytest.mark.parametrize("flag", ["W", "WW"])
def test_refined_tree_identical_to_reference(oracle_build, tmp_path, idx, flag):
    rec = WLS["trees"][idx]
    fa = write_family(tmp_path, rec)
    assert run(os.path.join(oracle_build, "pgmsa_oracle"), ["-T", "-i", "0", "-a", "-" + flag, fa]) == rec[flag]


@pytest.mark.parametrize("idx", range(len(WLS["fasta"])), ids=lambda i: "n%d" % WLS["fasta"][i]["n"])
def test_refined_fasta_identical_to_reference(oracle_build, tmp_path, idx):
    rec = WLS["fasta"][idx]
    fa = write_family(tmp_path, rec)
    out = run(os.path.join(oracle_build, "pgmsa_oracle"), ["--fasta", "-a", "-m", "-W", fa])
    key = "fasta/%d" % rec["n"]
    if key in KNOWN:   # (the reason is recorded next to the fixture): the same rows, only their order may differ
        assert sorted(out.split(">")) == sorted(rec["W"].split(">"))
    else:
        assert out == rec["W"]


def test_refinement_changes_the_tree(oracle_build, tmp_path):
    """-W is not a no-op on these families: the refined trees differ from the plain BioNJ trees."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    changed = 0
    for rec in WLS["trees"][:6]:
        fa = write_family(tmp_path, rec)
        changed += run(exe, ["-T", "-i", "0", "-a", fa]) != rec["W"]
    assert changed >= 4


def test_wls_flag_parsing_and_stats(oracle_build, tmp_path):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    rec = WLS["trees"][4]
    fa = write_family(tmp_path, rec)
    assert run(exe, ["-T", "-i", "0", "-a", "-W", "-W", fa]) == rec["WW"]
    assert run(exe, ["-T", "-i", "0", "-a", "--wls_refine", fa]) == rec["W"]
    r = subprocess.run([exe, "-T", "-i", "0", "-a", "-WW", "--stats", fa], capture_output=True, text=True)
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["wls_refine"] == 2 and stats["wls_trees"] == 1 and stats["wls_sweeps"] >= 2
    assert stats["wls_quartets"] > 0 and stats["wls_quintets"] > 0 and stats["wls_launches"] == 0
    r = subprocess.run([exe, "-T", "-i", "0", "-a", "--stats", fa], capture_output=True, text=True)
    assert "wls" not in r.stderr
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert "--wls_refine" in r.stderr


def test_wls_refines_every_tree_estimate(oracle_build, tmp_path):
    """With -i, every re-estimated tree is refined too (TreeNJ.h:52-54 on each path)."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    fa = write_family(tmp_path, WLS["fasta"][0])
    r = subprocess.run([exe, "-T", "-i", "2", "-W", "--stats", fa], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stderr.strip().splitlines()[-1])["wls_trees"] >= 2   # the first tree and at least one re-estimate


# ---- NNLS.h in numpy --------------------------------------------------------------------------------------------------
def nnls_reference(Z, x, TOL=1e-6, MAX_ITER=100):
    """The reference's active-set loop, line by line, with an SVD least-squares solve."""
    cols = Z.shape[1]
    lsq = lambda A: np.linalg.lstsq(A, x, rcond=None)[0]
    d = lsq(Z)
    if d.min() >= 0:
        return 0, d
    P = np.zeros(cols, bool)
    d = np.zeros(cols)
    w = Z.T @ (x - Z @ d) * (1.0 - P)
    n_iter = 0
    while not P.all() and w.max() > TOL:
        iw = int(np.argmax(w))
        P[iw] = True
        if n_iter > MAX_ITER:
            return n_iter + 1, d
        n_iter += 1
        while True:
            mapping = np.flatnonzero(P)
            iiw = int(np.flatnonzero(mapping == iw)[0])
            dp = d[mapping].copy()
            sp = lsq(Z[:, mapping])
            if sp.min() > 0:
                d[mapping] = sp
                w = Z.T @ (x - Z @ d) * (1.0 - P)
                break
            elif sp[iiw] <= 0:
                w[iw] = 0
                break
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = dp / (dp - sp)
            alpha[sp > 0] = np.inf
            ia = int(np.argmin(alpha))
            dp = dp + alpha[ia] * (sp - dp)
            for i in range(len(mapping)):
                if dp[i] <= 0 or i == ia:
                    P[mapping[i]] = False
                    d[mapping[i]] = 0
                else:
                    d[mapping[i]] = dp[i]
    return n_iter, d


QUARTET = np.array([[(m >> c) & 1 for c in range(5)] for m in (0x03, 0x15, 0x19, 0x16, 0x1A, 0x0C)], float)
QUINTET = np.array([[(m >> c) & 1 for c in range(7)] for m in (0x03, 0x65, 0x69, 0x31, 0x66, 0x6A, 0x32, 0x0C, 0x54, 0x58)], float)


def test_nnls_matches_numpy_statement(tmp_path):
    exe = str(tmp_path / "nnls_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "prographmsa_amd", "host"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "nnls_test.cpp")], check=True)
    rng = np.random.default_rng(7)
    probs = []
    for k in range(400):
        design = QUARTET if k % 2 == 0 else QUINTET
        Z = rng.uniform(0.2, 3.0, design.shape[0])[:, None] * design   # (weights on the rows, as Opt4 / Opt5 build A)
        if k % 4 < 2:
            Z = rng.normal(size=design.shape)                           # dense random 6 x 5 / 10 x 7
        x = rng.normal(0.3, 1.0, design.shape[0])
        probs.append((Z, x))
    text = "".join("%d %d %s %s\n" % (Z.shape[0], Z.shape[1], " ".join(repr(float(v)) for v in Z.ravel()), " ".join(repr(float(v)) for v in x))
                   for Z, x in probs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(probs)
    active = 0
    for (Z, x), line in zip(probs, lines):
        it, *d = line.split()
        d = np.array([float(v) for v in d])
        want_it, want = nnls_reference(Z, x)
        assert int(it) == want_it
        np.testing.assert_allclose(d, want, rtol=1e-9, atol=1e-12)
        assert (d >= 0).all() or want_it == 0
        active += want_it > 0
    assert active > 100   # most problems start with a negative entry and go through the active-set path
