"""Helpers of the --batch tests (tests/test_cpu_batch.py, tests/test_gpu_batch.py): seeded family sets, the list file, and the
comparison of every output of one `--batch` run with the stdout of the solo run of the same options on that family."""
import json
import os
import random
import subprocess

import numpy as np

import gen

SIZES = [2, 3, 5, 8, 13, 24]


def aa_families(d, sizes=SIZES, per_size=2, seed=1000):
    """per_size families of every size, 40-300 residues; the first family of 5 carries a start character on some rows (the strip /
    re-insert path).  Returns the FASTA paths in list order."""
    rng = random.Random(seed)
    out = []
    for n in sizes:
        for k in range(per_size):
            L = rng.randint(40, 300)
            seqs = gen.gen(n, L, seed + 17 * len(out))
            if n == 5 and k == 0:
                seqs = [("M" + s[1:]) if i % 2 == 0 else ("A" + s[1:]) for i, s in enumerate(seqs)]
            else:
                seqs = [("A" + s[1:]) if s[0] == "M" else s for s in seqs]
            p = os.path.join(str(d), "fam%02d_n%d.fa" % (len(out), n))
            with open(p, "w") as f:
                f.write(gen.fasta(seqs))
            out.append(p)
    return out


def dna_families(d, n_fam=4, seed=500):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_fam):
        n, L = int(rng.integers(3, 12)), int(rng.integers(60, 250))
        seqs = gen.gen(n, L, seed + k, alphabet="ACGT")
        p = os.path.join(str(d), "dna%02d.fa" % k)
        with open(p, "w") as f:
            f.write(gen.fasta(seqs))
        out.append(p)
    return out


def codon_families(d, n_fam=3, seed=700):
    out = []
    for k in range(n_fam):
        seqs = gen.gen_codon(4 + 3 * k, 30 + 20 * k, seed + k)
        if k == 1:
            seqs = ["ATG" + s[3:] if i % 2 else s for i, s in enumerate(seqs)]   # (start codons on some rows)
        p = os.path.join(str(d), "cod%02d.fa" % k)
        with open(p, "w") as f:
            f.write(gen.fasta(seqs))
        out.append(p)
    return out


def hky_model(d):
    """An HKY-like 4-state custom model file (lower triangle of the exchangeabilities in TCAG order, then the frequencies)."""
    p = os.path.join(str(d), "hky.model")
    with open(p, "w") as f:
        f.write("4.0 1.0 1.0 1.0 1.0 4.0 0.3 0.2 0.25 0.25\n")
    return p


def run(exe, args, env=None, code=0, timeout=300):
    """One driver run under a time limit of its own."""
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == code, (args, r.returncode, r.stderr[-2000:])
    return r


def solo_trees(exe, fams, opts, d, env=None):
    """The guide tree `exe -T -i 0` estimates for every family, written beside it."""
    trees = []
    for fa in fams:
        t = os.path.join(str(d), os.path.basename(fa) + ".nwk")
        with open(t, "w") as f:
            f.write(run(exe, list(opts) + ["-T", "-i", "0", fa], env).stdout)
        trees.append(t)
    return trees


def write_list(path, fams, outs, trees=None):
    with open(path, "w") as f:
        f.write("# input<TAB>output[<TAB>tree]\n\n")
        for i, fa in enumerate(fams):
            cols = [fa, outs[i]] + ([trees[i]] if trees is not None and trees[i] else [])
            f.write("\t".join(cols) + "\n")


def stats_of(stderr):
    lines = [l for l in stderr.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stderr[-2000:]
    return json.loads(lines[0])


def run_batch(exe, fams, opts, d, tag, trees=None, env=None, extra=(), code=0):
    """One `--batch` run; returns (output paths, the --stats record, stderr)."""
    outs = [os.path.join(str(d), "%s_%02d.out" % (tag, i)) for i in range(len(fams))]
    lst = os.path.join(str(d), tag + ".list")
    write_list(lst, fams, outs, trees)
    r = run(exe, ["--batch", lst, "--stats"] + list(opts) + list(extra), env, code)
    return outs, stats_of(r.stderr), r.stderr


def solo_outputs(exe, fams, opts, trees=None, env=None):
    res = []
    for i, fa in enumerate(fams):
        t = ["-t", trees[i]] if trees is not None and trees[i] else []
        res.append(run(exe, list(opts) + t + [fa], env).stdout)
    return res


def assert_identical(outs, solo):
    assert len(outs) == len(solo)
    for p, s in zip(outs, solo):
        assert os.path.exists(p), p
        with open(p) as f:
            got = f.read()
        assert len(s) > 0
        assert got == s, "%s differs from the solo run" % p


def tree_height(newick):
    """Height (longest path of internal nodes to a leaf) of a newick tree: the levels a progressive pass over it has."""
    depth = best = 0
    for c in newick:
        if c == "(":
            depth += 1
            best = max(best, depth)
        elif c == ")":
            depth -= 1
    return best
