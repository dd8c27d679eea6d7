"""DNA alignment (--dna), custom rate models (--custom_model) and estimated frequencies (-F / -C) through the CPU oracle driver.

The DNA alphabet is the reference's intended one (T=0 C=1 A=2 G=3, unknown 4: DESIGN.md §0), not its DNA::value(), so there is
no reference output to pin: the alphabet, the models and the k-mer angle distances are checked against numpy statements of
ModelFactoryCustom.h, ModelFactoryPlusF.h and DistanceFactoryAngle.h."""
import os
import subprocess

import numpy as np
import pytest

from prographmsa_amd import jobs as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NT = "TCAG"
AA = "ACDEFGHIKLMNPQRSTVWY"
UNKNOWN = set("XNRYSWKMBDHV")


def run(exe, args, code=0):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == code, (r.returncode, r.stderr)
    return r.stdout if code == 0 else r.stderr


def oracle(build):
    return os.path.join(build, "pgmsa_oracle")


def read_fasta(text):
    out, name = {}, None
    for line in text.splitlines():
        if line.startswith(">"):
            name = line[1:].strip()
            out[name] = ""
        elif name is not None:
            out[name] += line.strip()
    return out


def dna_family(n, L, seed, sub=0.08, ts_bias=0.7, indel=0.02, n_frac=0.002, case=False):
    """n sequences evolved from one random root: substitutions (a transition with probability ts_bias), short indels and a few
    N.  Returns (fasta text, {name: sequence})."""
    rng = np.random.default_rng(seed)
    ts = {"A": "G", "G": "A", "C": "T", "T": "C"}
    root = list(rng.choice(list("ACGT"), L))
    seqs = {}
    for i in range(n):
        s = []
        for c in root:
            r = rng.random()
            if r < indel / 2:
                continue                                            # deletion
            if r < indel:
                s.extend(rng.choice(list("ACGT"), int(rng.integers(1, 4))))   # insertion
            if rng.random() < sub:
                c = ts[c] if rng.random() < ts_bias else rng.choice([x for x in "ACGT" if x != c and x != ts[c]])
            if rng.random() < n_frac:
                c = "N"
            s.append(c)
        s = "".join(s)
        if case and i % 3 == 1:
            s = s.lower()
        seqs["d%03d" % i] = s
    return "".join(">%s\n%s\n" % kv for kv in seqs.items()), seqs


def model_text(S, f):
    D = len(f)
    vals = [S[i, j] for i in range(1, D) for j in range(i)] + list(f)
    return " ".join(repr(float(v)) for v in vals) + "\n"


def random_model(D, seed):
    rng = np.random.default_rng(seed)
    S = rng.uniform(0.2, 3.0, (D, D))
    S = np.triu(S, 1) + np.triu(S, 1).T
    f = rng.uniform(0.5, 2.0, D)
    return S, f


HKY = (np.array([[0, 4.0, 1.0, 1.0], [4.0, 0, 1.0, 1.0], [1.0, 1.0, 0, 4.0], [1.0, 1.0, 4.0, 0]]), np.array([0.3, 0.2, 0.25, 0.25]))


# ---- numpy statements ---------------------------------------------------------------------------------------------------
def normalise(Q, f):
    """Diagonal reset and rate normalisation (ModelFactoryCustom.h:62-65)."""
    Q = Q.copy()
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    return Q / -(f @ np.diag(Q))


def custom_Q(S, f):
    f = np.asarray(f, float) / np.sum(f)
    return normalise(np.asarray(S, float), f), f


def plusF(Q0, f0, counts, N):
    """ModelFactoryPlusF.h:72-105: f = (f0 N + counts) / sum, Q = Q0 diag(f / f0), renormalised."""
    f = f0 * N + counts
    f = f / f.sum()
    return normalise(Q0 @ np.diag(f / f0), f), f


def expm_reversible(Q, w, t):
    """exp(Q t) for Q reversible with respect to w (w_i Q_ij = w_j Q_ji): symmetrised, then numpy.linalg.eigh."""
    s = np.sqrt(w)
    B = s[:, None] * Q / s[None, :]
    B = (B + B.T) / 2
    lam, U = np.linalg.eigh(B)
    return (U / s[:, None]) @ np.diag(np.exp(lam * t)) @ (U.T * s[None, :])


def model_distance(d):
    """ModelFactory::parseDistance without -m / -M, and the [min_dist, max_dist] clamp."""
    md = 5.2 if d > 0.85 else -np.log(1.0 - d - 0.2 * d * d)
    return min(max(md, 0.05), 2.2)


def dumped_job(exe, tmp_path, fa_text, flags, bl):
    """The single alignGraphs job of a two-sequence family on the tree (a:bl0, b:bl1): its M (dim x dim) and pi."""
    fa = tmp_path / "two.fa"
    fa.write_text(fa_text)
    tree = tmp_path / "two.tree"
    names = [l[1:].strip() for l in fa_text.splitlines() if l.startswith(">")]
    tree.write_text("(%s:%r,%s:%r);\n" % (names[0], bl[0], names[1], bl[1]))
    dump = tmp_path / "jobs.bin"
    if dump.exists():
        dump.unlink()
    run(exe, flags + ["-f", "-t", str(tree), "--dump_jobs", str(dump), str(fa)])
    js = J.load_jobs(str(dump))
    assert len(js) == 1
    d = js[0].g1.dim
    return np.asarray(js[0].M).reshape(d, d, order="F"), np.asarray(js[0].pi), model_distance(bl[0] + bl[1])


def assert_close(a, b, rel=1e-12):
    assert np.max(np.abs(a - b)) <= rel * np.max(np.abs(b)), np.max(np.abs(a - b)) / np.max(np.abs(b))


# ---- alphabet -----------------------------------------------------------------------------------------------------------
def test_alphabet_values_output_and_case(oracle_build, tmp_path):
    """TCAG values, U as T, N / X / IUPAC as unknown (uniform columns), the input's own characters (case included) in the
    output, every row without its gaps equal to its input."""
    text, seqs = dna_family(12, 300, 5, case=True)
    seqs["d001"] = seqs["d001"][:40] + "RYSWKMBDHVNXrysw" + seqs["d001"][40:]
    seqs["d002"] = seqs["d002"].replace("T", "U").replace("t", "u")
    text = "".join(">%s\n%s\n" % kv for kv in seqs.items())
    (tmp_path / "f.fa").write_text(text)
    (tmp_path / "m").write_text(model_text(*HKY))
    out = read_fasta(run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m"), "-f", str(tmp_path / "f.fa")]))
    assert set(out) == set(seqs)
    assert len({len(v) for v in out.values()}) == 1
    for k, v in out.items():
        assert v.replace("-", "") == seqs[k]
    assert any(c.islower() for c in out["d001"] + out["d004"])
    assert "U" in out["d002"] and "T" not in out["d002"].upper()


def test_dna_values_in_the_jobs(oracle_build, tmp_path):
    """A leaf's profile column is one-hot at the TCAG value of its residue (U = T, either case) and uniform 1/4 for N and
    the ambiguity letters."""
    s1 = "TCAGUtcagu" + "".join(sorted(UNKNOWN)) + "n"
    s2 = "ACGT" * 5
    (tmp_path / "m").write_text(model_text(*HKY))
    fa = ">a\n%s\n>b\n%s\n" % (s1, s2)
    (tmp_path / "two.fa").write_text(fa)
    (tmp_path / "two.tree").write_text("(a:0.1,b:0.1);\n")
    run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m"), "-f", "-t", str(tmp_path / "two.tree"),
                               "--dump_jobs", str(tmp_path / "j.bin"), str(tmp_path / "two.fa")])
    j = J.load_jobs(str(tmp_path / "j.bin"))[0]
    g = j.g1 if j.g1.n == len(s1) + 2 else j.g2
    cols = np.asarray(g.sites).reshape(g.n, 4)[1:-1]
    for c, col in zip(s1, cols):
        exp = np.full(4, 0.25) if c.upper() in UNKNOWN else np.eye(4)[NT.index(c.upper().replace("U", "T"))]
        assert np.array_equal(col, exp), c


def test_identical_sequences_align_without_gaps(oracle_build, tmp_path):
    rng = np.random.default_rng(3)
    s = "".join(rng.choice(list("ACGT"), 250))
    (tmp_path / "f.fa").write_text("".join(">s%d\n%s\n" % (i, s) for i in range(6)))
    (tmp_path / "m").write_text(model_text(*HKY))
    out = read_fasta(run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m"), "-f", str(tmp_path / "f.fa")]))
    assert all(v == s for v in out.values())


@pytest.mark.parametrize("bad", ["ACGTE", "ACG*T", "AC1GT", "ACGTJ"])
def test_bad_characters_are_refused(oracle_build, tmp_path, bad):
    (tmp_path / "f.fa").write_text(">a\n%s\n>b\nACGTACGT\n>c\nACGTTT\n" % bad)
    (tmp_path / "m").write_text(model_text(*HKY))
    err = run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m"), "-f", str(tmp_path / "f.fa")], code=2)
    assert "invalid character" in err


def test_gapped_input_is_refused(oracle_build, tmp_path):
    (tmp_path / "f.fa").write_text(">a\nAC-GT\n>b\nACGTACGT\n>c\nACGTTT\n")
    (tmp_path / "m").write_text(model_text(*HKY))
    err = run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m"), "-f", str(tmp_path / "f.fa")], code=2)
    assert "No support for gapped sequences (yet)" in err


# ---- models -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", ["dna", "aa"])
@pytest.mark.parametrize("bl", [(0.02, 0.03), (0.1, 0.25), (0.3, 0.35), (0.6, 0.7)])
def test_custom_model_M_and_pi(oracle_build, tmp_path, alphabet, bl):
    """file -> Q (symmetric exchangeabilities, diagonal -row sum, rate 1 under pi) -> P(d) = expm(Q d) -> M = diag(pi) P(d)."""
    D = 4 if alphabet == "dna" else 20
    S, f = random_model(D, 11 + D)
    (tmp_path / "m").write_text(model_text(S, f))
    if alphabet == "dna":
        fa = ">a\nACGTTGCAACGTAGCT\n>b\nACGTAGCAACCTAGCT\n"
        flags = ["--dna"]
    else:
        fa = ">a\nACDEFGHIKLMNPQRSTVWY\n>b\nACDEFGHKKLMNPQRSTVWY\n"
        flags = []
    M, pi, d = dumped_job(oracle(oracle_build), tmp_path, fa, flags + ["--custom_model", str(tmp_path / "m")], bl)
    Q, fn = custom_Q(S, f)
    assert np.allclose(Q, Q.T, rtol=0, atol=1e-15)
    assert_close(pi, fn)
    assert_close(M, np.diag(fn) @ expm_reversible(Q, np.ones(D), d))


def residue_counts(seqs, alphabet):
    D = len(alphabet)
    c = np.zeros(D)
    for s in seqs:
        for ch in s.upper().replace("U", "T"):
            if ch in alphabet:
                c[alphabet.index(ch)] += 1
    return c


@pytest.mark.parametrize("N", [1000.0, 10.0, 0.5])
@pytest.mark.parametrize("alphabet", ["dna", "aa"])
def test_estimated_frequencies(oracle_build, tmp_path, alphabet, N):
    """-F / -C: f = (pi_base N + residue counts) / sum, Q = Q_base diag(f / pi_base), renormalised; M from that Q."""
    D = 4 if alphabet == "dna" else 20
    S, f0 = random_model(D, 21 + D)
    (tmp_path / "m").write_text(model_text(S, f0))
    rng = np.random.default_rng(7)
    if alphabet == "dna":
        a = "".join(rng.choice(list("AAAACGTTN"), 300))
        b = "".join(rng.choice(list("ACGGGGT"), 280))
        flags = ["--dna"]
    else:
        a = "".join(rng.choice(list(AA + "LLLLX"), 300))
        b = "".join(rng.choice(list(AA + "WWW"), 280))
        flags = []
    args = flags + ["--custom_model", str(tmp_path / "m"), "-F"] + ([] if N == 1000.0 else ["-C", repr(N)])
    M, pi, d = dumped_job(oracle(oracle_build), tmp_path, ">a\n%s\n>b\n%s\n" % (a, b), args, (0.2, 0.15))
    Q0, fb = custom_Q(S, f0)
    Q, f = plusF(Q0, fb, residue_counts([a, b], NT if alphabet == "dna" else AA), N)
    assert_close(pi, f)
    assert_close(M, np.diag(f) @ expm_reversible(Q, f / fb, d))
    if N == 0.5:
        assert np.max(np.abs(f - fb)) > 1e-3   # (the estimate moved the frequencies)


def test_estimated_frequencies_change_the_alignment_input(oracle_build, tmp_path):
    """-F on the default amino-acid model (WAG) runs and changes the model the jobs are given."""
    fa = os.path.join(GOLD, "c1.fa")
    tree = os.path.join(GOLD, "c1.tree")
    ms = []
    for flags in ([], ["-F"]):
        dump = tmp_path / ("j%d.bin" % len(flags))
        run(oracle(oracle_build), flags + ["-f", "-t", tree, "--dump_jobs", str(dump), fa])
        ms.append(np.asarray(J.load_jobs(str(dump))[0].pi))
    assert not np.array_equal(ms[0], ms[1]) and abs(ms[1].sum() - 1) < 1e-12


# ---- k-mer angle distances (K = 6) ----------------------------------------------------------------------------------------
def kmer_counts(s, K=6):
    v = [NT.index(c) if c in NT else -1 for c in s.upper().replace("U", "T")]
    c = np.zeros(4 ** K)
    for j in range(K - 1, len(v)):
        w = v[j - K + 1:j + 1]
        if min(w) >= 0:
            c[int(np.dot(w, 4 ** np.arange(K - 1, -1, -1)))] += 1
    return c


@pytest.mark.parametrize("ml", [False, True])
def test_angle_distances_k6(oracle_build, tmp_path, ml):
    text, seqs = dna_family(20, 400, 9, n_frac=0.01)
    (tmp_path / "f.fa").write_text(text)
    (tmp_path / "m").write_text(model_text(*HKY))
    dump = tmp_path / "dist.bin"
    run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m"), "-T", "-i", "0", "--dump_dist", str(dump)]
        + (["-m"] if ml else []) + [str(tmp_path / "f.fa")])
    buf = dump.read_bytes()
    n = int(np.frombuffer(buf, np.int32, 1)[0])
    assert len(buf) == 4 + 16 * n * n
    Dm = np.frombuffer(buf, np.float64, n * n, 4).reshape(n, n)
    Vm = np.frombuffer(buf, np.float64, n * n, 4 + 8 * n * n).reshape(n, n)
    names = sorted(seqs)
    C = np.array([kmer_counts(seqs[k]) for k in names])
    inv = 1.0 / np.sqrt((C * C).sum(1))
    cos = (C * inv[:, None]) @ C.T * inv[None, :]
    d = -np.log((cos ** 2 + 0.4) / 1.4)
    if not ml:
        e = np.exp(d)
        d = -0.5 * (5.0 * e - np.sqrt(45.0 * e * e - 20.0 * e)) / e
    lens = np.array([len(seqs[k]) for k in names], float)
    v = np.maximum(d / ((lens[:, None] + lens[None, :]) / 2), 1e-5)
    assert np.allclose(Dm, d, rtol=1e-12, atol=1e-12)
    assert np.allclose(Vm, v, rtol=1e-12, atol=1e-12)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_dna_needs_a_custom_model(oracle_build, tmp_path):
    (tmp_path / "f.fa").write_text(dna_family(4, 50, 1)[0])
    err = run(oracle(oracle_build), ["--dna", "-f", str(tmp_path / "f.fa")], code=2)
    assert "custom model file necessary for DNA alignments" in err


@pytest.mark.parametrize("other", [["--codon"], ["-c", os.path.join(GOLD, "K50.lib")]])
def test_dna_refuses_codon_and_cs_profiles(oracle_build, tmp_path, other):
    (tmp_path / "f.fa").write_text(dna_family(4, 60, 1)[0])
    (tmp_path / "m").write_text(model_text(*HKY))
    err = run(oracle(oracle_build), ["--dna", "--custom_model", str(tmp_path / "m")] + other + ["-f", str(tmp_path / "f.fa")], code=2)
    assert "--dna cannot be combined" in err


@pytest.mark.parametrize("case,msg", [
    ("zero_rate", "negative/infinity/zero value in exchangeability matrix"),
    ("negative_rate", "negative/infinity/zero value in exchangeability matrix"),
    ("missing_rate", "error reading amino acid frequencies"),
    ("text_rate", "error reading exchangeability matrix from file"),
    ("zero_freq", "negative/infinity/zero value in amino acid frequencies"),
    ("negative_freq", "negative/infinity/zero value in amino acid frequencies"),
    ("missing_freq", "error reading amino acid frequencies"),
    ("no_file", "error reading exchangeability matrix from file"),
])
def test_bad_model_files_are_refused(oracle_build, tmp_path, case, msg):
    vals = ["1.0", "4.0", "1.0", "1.0", "4.0", "1.0", "0.3", "0.2", "0.25", "0.25"]
    if case == "zero_rate": vals[2] = "0"
    if case == "negative_rate": vals[4] = "-1.5"
    if case == "missing_rate": vals = vals[:5] + vals[6:]   # (one value short: the last frequency is missing)
    if case == "text_rate": vals[1] = "abc"
    if case == "zero_freq": vals[7] = "0.0"
    if case == "negative_freq": vals[9] = "-0.25"
    if case == "missing_freq": vals = vals[:-1]
    m = tmp_path / "m"
    if case != "no_file":
        m.write_text(" ".join(vals) + "\n")
    (tmp_path / "f.fa").write_text(dna_family(4, 60, 1)[0])
    err = run(oracle(oracle_build), ["--dna", "--custom_model", str(m), "-f", str(tmp_path / "f.fa")], code=2)
    assert msg in err


def test_help_lists_the_new_flags(oracle_build):
    r = subprocess.run([oracle(oracle_build), "--help"], capture_output=True, text=True)
    for flag in ["--dna", "--custom_model", "--estimate_aafreqs", "--aafreqs_pseudocount", "-F", "-C", "ACDEFGHIKLMNPQRSTVWY"]:
        assert flag in r.stderr, flag
