"""Helpers of the --guidance tests (tests/test_cpu_guidance.py, tests/test_gpu_guidance.py): the five family kinds, one driver run
with its files, and the scores restated in numpy from the written FASTA files alone (a brute-force compare over all (r, i, j, c))."""
import os
import re

import numpy as np

import batch_util as bu
import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KINDS = ["aa", "codon", "dna", "repeats", "cs"]


def families(d):
    """{kind: (fasta path, options)}: amino acids (13 taxa, start characters on some rows), codons (start codons on some rows),
    DNA with a custom model, a family with annotated tandem repeats, and amino acids with a context-profile library."""
    d = str(d)
    out = {}

    def put(kind, name, seqs, opts):
        p = os.path.join(d, name)
        with open(p, "w") as f:
            f.write(gen.fasta(seqs))
        out[kind] = (p, opts)

    aa = gen.gen(13, 110, 4242)
    put("aa", "aa.fa", [("M" + s[1:]) if i % 3 == 0 else ("A" + s[1:]) for i, s in enumerate(aa)], [])
    cod = gen.gen_codon(7, 50, 701)
    put("codon", "cod.fa", ["ATG" + s[3:] if i % 2 else s for i, s in enumerate(cod)], ["--codon"])
    put("dna", "dna.fa", gen.gen(9, 120, 503, alphabet="ACGT"), ["--dna", "--custom_model", bu.hky_model(d)])
    seqs, trd = gen.gen_repeat_family(8, 90, 3)
    with open(os.path.join(d, "r.trd"), "w") as f:
        f.write(trd)
    put("repeats", "rep.fa", seqs, ["--read_repeats", os.path.join(d, "r.trd")])
    put("cs", "cs.fa", [("A" + s[1:]) if s[0] == "M" else s for s in gen.gen(6, 80, 77)], ["-c", os.path.join(GOLD, "K50.lib")])
    return out


class Run:
    pass


def guidance(exe, fa, d, tag, n=6, opts=(), seed=None, residues=True, dump=True, env=None):
    """One `--guidance` run: stdout, the two files, the dumped trees and alignments (texts), the --stats record."""
    d = str(d)
    r = Run()
    r.out_path = os.path.join(d, tag + ".tsv")
    r.res_path = os.path.join(d, tag + ".res.tsv")
    r.prefix = os.path.join(d, tag + ".rep")
    args = ["--fasta", "--stats", "--guidance", str(n), "--guidance_out", r.out_path]
    if seed is not None:
        args += ["--guidance_seed", str(seed)]
    if residues:
        args += ["--guidance_residues", r.res_path]
    if dump:
        args += ["--guidance_dump", r.prefix]
    p = bu.run(exe, args + list(opts) + [fa], env)
    r.stdout, r.stats = p.stdout, bu.stats_of(p.stderr)
    r.out = open(r.out_path).read()
    r.res = open(r.res_path).read() if residues else None
    r.trees = [open("%s.%d.nwk" % (r.prefix, k)).read() for k in range(n)] if dump else None
    r.alns = [open("%s.%d.fa" % (r.prefix, k)).read() for k in range(n)] if dump else None
    return r


def read_fasta(text):
    out, name = {}, None
    for line in text.splitlines():
        if line.startswith(">"):
            name = line[1:]
            out[name] = ""
        else:
            out[name] += line
    return out


def symbols(row, w):
    assert len(row) % w == 0
    return [row[k:k + w] for k in range(0, len(row), w)]


def where_of(base, rep, names, w):
    """where[i][c] of one replicate from the two written alignments: the k-th residue of a row stands in the k-th column without a
    gap of either alignment."""
    L = len(base[names[0]]) // w
    out = np.full((len(names), L), -1, np.int32)
    for i, s in enumerate(names):
        b, r = symbols(base[s], w), symbols(rep[s], w)
        pos = [k for k, x in enumerate(r) if x != "-" * w]
        cols = [c for c, x in enumerate(b) if x != "-" * w]
        assert len(pos) == len(cols) and [b[c] for c in cols] == [r[k] for k in pos], s
        out[i, cols] = pos
    return out


def agreement(where):
    """res_hits (nrows x ncols) and pair_hits (nrows x nrows) of where (nrep x nrows x ncols), by comparing everything."""
    where = np.asarray(where)
    nrep, n, L = where.shape
    res = np.zeros((n, L), np.int64)
    pair = np.zeros((n, n), np.int64)
    for r in range(nrep):
        w = where[r]
        hit = (w[:, None, :] == w[None, :, :]) & (w[:, None, :] >= 0)     # (i, j, c)
        hit[np.arange(n), np.arange(n), :] = False
        res += hit.sum(axis=1)
        pair += hit.sum(axis=2)
    return res, pair


def _line(hits, pairs):
    return "%d\t%d\t%s\n" % (hits, pairs, ("%.6f" % (float(hits) / float(pairs))) if pairs else "NA")


def expected_files(base_text, rep_texts, w, seed):
    """The texts of --guidance_out and --guidance_residues from the written base alignment and the replicates' alignments."""
    base = read_fasta(base_text)
    names = sorted(s for s in base if not s.startswith("("))
    where = np.array([where_of(base, read_fasta(t), names, w) for t in rep_texts])
    N, n, L = where.shape
    res, pair = agreement(where)
    has = where[0] >= 0
    occ = has.sum(axis=0)
    out = ["# guidance replicates=%d seed=%d sequences=%d columns=%d\n" % (N, seed, n, L)]
    chits = [int(res[:, c].sum()) // 2 for c in range(L)]
    cpairs = [N * int(occ[c]) * (int(occ[c]) - 1) // 2 for c in range(L)]
    out.append("alignment\t" + _line(sum(chits), sum(cpairs)))
    out += ["column\t%d\t" % (c + 1) + _line(chits[c], cpairs[c]) for c in range(L)]
    for i, s in enumerate(names):
        out.append("sequence\t%s\t" % s + _line(int(res[i].sum()), N * int((occ[has[i]] - 1).sum())))
    for i in range(n):
        for j in range(i + 1, n):
            out.append("pair\t%s\t%s\t" % (names[i], names[j]) + _line(int(pair[i, j]), N * int((has[i] & has[j]).sum())))
    resid = []
    for i, s in enumerate(names):
        for c in range(L):
            if has[i, c]:
                resid.append("%s\t%d\t" % (s, c + 1) + _line(int(res[i, c]), N * (int(occ[c]) - 1)))
    return "".join(out), "".join(resid)


def column_scores(out_text):
    """{column (from 1): score or None} of a --guidance_out text."""
    cols = {}
    for line in out_text.splitlines():
        f = line.split("\t")
        if f[0] == "column":
            cols[int(f[1])] = None if f[4] == "NA" else float(f[4])
    return cols


# ---- newick with branch lengths -----------------------------------------------------------------------------------------
_TOKEN = re.compile(r"[^,:();]+")


def parse_newick(text):
    """A tree as nested nodes: a leaf is its name, an internal node a list of (child, branch length)."""
    pos = 0

    def node():
        nonlocal pos
        if text[pos] != "(":
            m = _TOKEN.match(text, pos)
            pos = m.end()
            return m.group(0)
        pos += 1
        kids = []
        while True:
            kid = node()
            assert text[pos] == ":"
            m = _TOKEN.match(text, pos + 1)
            pos = m.end()
            kids.append((kid, float(m.group(0))))
            if text[pos] == ",":
                pos += 1
                continue
            assert text[pos] == ")"
            pos += 1
            return kids

    root = node()
    assert text[pos:].strip() == ";"
    return root


def leaf_depths(node):
    """{leaf: distance to `node`}"""
    if isinstance(node, str):
        return {node: 0.0}
    out = {}
    for kid, length in node:
        for s, dpt in leaf_depths(kid).items():
            out[s] = dpt + length
    return out


def longest_path(node):
    """The longest leaf-to-leaf path of the tree below `node`."""
    if isinstance(node, str):
        return 0.0
    best = max(longest_path(kid) for kid, _ in node)
    tops = sorted((max(leaf_depths(kid).values()) + length for kid, length in node), reverse=True)
    return max(best, tops[0] + tops[1]) if len(tops) > 1 else best


def splits_of(root):
    """The non-trivial bipartitions of a tree: the side without the first leaf in sorted-name order, as frozensets of names."""
    names = sorted(leaf_depths(root))
    everything = frozenset(names)
    out = set()

    def walk(node):
        if isinstance(node, str):
            return frozenset([node])
        below = frozenset()
        for kid, _ in node:
            below |= walk(kid)
        side = everything - below if names[0] in below else below
        if 2 <= len(side) <= len(names) - 2:
            out.add(side)
        return below

    walk(root)
    return names, out
