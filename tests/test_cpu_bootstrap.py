"""`--bootstrap` through the CPU oracle driver (pgmsa_oracle: the Backend default gathers every replicate on the host and counts it
with the oracle's pair-count loop): the refusals, the file against the tree `-T` prints, the labels, the support counter on
hand-written trees (tests/native/bootstrap_test.cpp), and the whole flow restated in Python for p-distances: splitmix64, the
gather, pgmo_prealigned_counts, the p-distance, BioNJ (bionj_ref) and the bipartition count."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_util as bu
import bionj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = re.compile(r"\)(\d+):")
MASK = (1 << 64) - 1


def strip_labels(text):
    return LABEL.sub("):", text)


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    all_fams = bu.aa_families(tmp_path_factory.mktemp("boot_fams"))
    pick = lambda n: next(f for f in all_fams if f.endswith("_n%d.fa" % n))
    return {n: pick(n) for n in (3, 5, 13, 24)}


def bootstrap(exe, fa, out, n=8, opts=(), seed=None, env=None):
    args = ["--fasta", "--stats", "--bootstrap", str(n), "--bootstrap_out", out] + (["--bootstrap_seed", str(seed)] if seed is not None else [])
    r = bu.run(exe, args + list(opts) + [fa], env)
    with open(out) as f:
        text = f.read()
    assert text.endswith(";\n") and text.count("\n") == 1
    return text, r


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(exe, fams, tmp_path):
    out = str(tmp_path / "never.nwk")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fams[5]], [str(tmp_path / "b.out")])
    topo = str(tmp_path / "topo.nwk")
    with open(topo, "w") as f:
        f.write(bu.run(exe, ["-T", "-i", "0", fams[5]]).stdout)
    both = ["--bootstrap", "4", "--bootstrap_out", out]
    cases = [
        ["--bootstrap", "4", fams[5]],                       # one without the other
        ["--bootstrap_out", out, fams[5]],
        ["--bootstrap", "0", "--bootstrap_out", out, fams[5]],      # N out of range
        ["--bootstrap", "1001", "--bootstrap_out", out, fams[5]],
        ["--bootstrap", "-3", "--bootstrap_out", out, fams[5]],
        both + [fams[3]],                                    # fewer than 4 sequences
        both + ["--batch", lst],
        ["--bootstrap", "4", "--batch", lst],
        both + ["-W", fams[5]],
        both + ["-r", fams[5]],
        both + ["--topology", topo, fams[5]],
    ]
    for args in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and r.stdout == "", (args, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "b.out")), args


# ---- the file ---------------------------------------------------------------------------------------------------------
def parse_labelled(text):
    """The tree of a labelled newick line: (children | leaf name, label or None) per node, root first."""
    pos = 0

    def node():
        nonlocal pos
        if text[pos] != "(":
            m = re.compile(r"[^,:()]+").match(text, pos)
            pos = m.end()
            return m.group(0), None
        pos += 1
        kids = []
        while True:
            kid = node()
            m = re.compile(r":[^,()]+").match(text, pos)
            pos = m.end()
            kids.append(kid)
            if text[pos] == ",":
                pos += 1
                continue
            assert text[pos] == ")"
            pos += 1
            break
        m = re.compile(r"\d*").match(text, pos)
        pos = m.end()
        return kids, (int(m.group(0)) if m.group(0) else None)

    root = node()
    assert text[pos:] == ";\n"
    return root


def leaves_of(n):
    return [n[0]] if isinstance(n[0], str) else [x for k in n[0] for x in leaves_of(k)]


def labelled_splits(root):
    """{canonical side (frozenset of leaf indices in sorted-name order, without leaf 0): [labels of the nodes with that split]}"""
    names = sorted(leaves_of(root))
    ix = {s: k for k, s in enumerate(names)}
    everything = frozenset(range(len(names)))
    out = {}

    def walk(n, is_root):
        if isinstance(n[0], str):
            assert n[1] is None
            return
        for k in n[0]:
            walk(k, False)
        if is_root:
            assert n[1] is None
            return
        side = frozenset(ix[s] for s in leaves_of(n))
        if 0 in side:
            side = everything - side
        if 2 <= len(side) <= len(names) - 2:
            assert n[1] is not None, "an internal edge without a label"
            out.setdefault(side, []).append(n[1])
        else:
            assert n[1] is None, "a label on a trivial bipartition"

    walk(root, True)
    return names, out


@pytest.mark.parametrize("n,opts", [(5, []), (13, []), (24, []), (13, ["-m"])], ids=["n5", "n13", "n24", "n13_m"])
def test_file_is_the_reestimated_tree_with_labels(exe, fams, tmp_path, n, opts):
    N = 8
    text, r = bootstrap(exe, fams[n], str(tmp_path / "b.nwk"), N, ["-i", "0"] + opts)
    assert strip_labels(text) == bu.run(exe, ["-T", "-i", "1"] + opts + [fams[n]]).stdout
    assert r.stdout == bu.run(exe, ["--fasta", "-i", "0"] + opts + [fams[n]]).stdout          # stdout as without the flags
    st = bu.stats_of(r.stderr)
    assert st["bootstrap_replicates"] == N and st["bootstrap_counts_calls"] == 1 and st["bootstrap_s"] > 0
    root = parse_labelled(text)
    names, splits = labelled_splits(root)
    assert len(names) == n and len(splits) == n - 3                      # every internal edge of a binary tree
    for labels in splits.values():
        assert all(0 <= v <= N for v in labels) and len(set(labels)) == 1 and len(labels) <= 2
    kids = root[0]
    assert len(kids) == 2
    if all(not isinstance(k[0], str) for k in kids):                      # the two root edges are one bipartition
        assert kids[0][1] == kids[1][1]


def test_only_tree_and_seeds(exe, fams, tmp_path):
    """-T prints what it prints without the flags (the final alignment is computed for the bootstrap alone); the same seed gives the
    same file, the default seed is 1, another seed another resampling."""
    a, r = bootstrap(exe, fams[24], str(tmp_path / "a.nwk"), 8, ["-T"])
    assert r.stdout == bu.run(exe, ["-T", fams[24]]).stdout
    b, _ = bootstrap(exe, fams[24], str(tmp_path / "b.nwk"), 8, ["-T"])
    c, _ = bootstrap(exe, fams[24], str(tmp_path / "c.nwk"), 8, ["-T"], seed=1)
    assert a == b == c
    hc, _ = bootstrap(exe, fams[24], str(tmp_path / "hc.nwk"), 8, ["-T"], env=dict(os.environ, PGM_HOST_COUNTS="1"))
    assert hc == a                                                        # the host's scan of the gathered rows: the same integers
    others = [bootstrap(exe, fams[24], str(tmp_path / ("s%d.nwk" % s)), 8, ["-T"], seed=s)[0] for s in (2, 3, 2 ** 63 + 5)]
    assert all(strip_labels(o) == strip_labels(a) for o in others) and any(o != a for o in others)


# ---- the counter on hand-written trees --------------------------------------------------------------------------------
def test_support_counter_native(tmp_path):
    exe = str(tmp_path / "bootstrap_test")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", host, "-o", exe, os.path.join(ROOT, "tests", "native", "bootstrap_test.cpp"),
                    os.path.join(host, "phytree.cpp"), os.path.join(host, "alphabet.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


# ---- the flow restated ------------------------------------------------------------------------------------------------
def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def resampled_columns(seed, nrep, ncols):
    cols = np.zeros((nrep, ncols), np.uint32)
    state = seed
    for r in range(nrep):
        for c in range(ncols):
            state, z = splitmix64(state)
            cols[r, c] = z % ncols
    return cols


def test_python_restatement_of_the_p_distance_flow(exe, fams, tmp_path):
    """DESIGN 3.13 step by step on the 13-taxon family, N = 6, seed 77: the labels of the file are the counts this gives."""
    import oracle_lib
    N, seed = 6, 77
    text, r = bootstrap(exe, fams[13], str(tmp_path / "b.nwk"), N, ["-i", "0"], seed=seed)
    aln = {}
    for line in r.stdout.splitlines():
        if line.startswith(">"):
            name = line[1:]
            aln[name] = ""
        else:
            aln[name] += line
    names = sorted(aln)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    rows = np.array([[(-1 if ch == "-" else aa.find(ch) if ch in aa else -2) for ch in aln[s]] for s in names], np.int8)
    n, L = rows.shape
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pi = np.array([p[0] for p in pairs], np.uint32)
    pj = np.array([p[1] for p in pairs], np.uint32)
    cols = resampled_columns(seed, N, L)
    found = []
    for rep in range(N):
        gathered = np.ascontiguousarray(rows[:, cols[rep]])
        counts, _ = oracle_lib.prealigned_counts(20, gathered, pi, pj)
        counts = np.asarray(counts).reshape(len(pairs), 20, 20)
        D = np.zeros((n, n))
        V = np.zeros((n, n))
        for p, (i, j) in enumerate(pairs):   # DistanceFactoryML::computeDistance without -m / -M, amino acids
            total = float(counts[p].sum())
            ident = float(np.trace(counts[p]))
            if total == 0:
                d, v = 1.0, 1e3
            else:
                d = 1.0 - ident / total
                v = d / total
            if not d < 2.2:
                d, v = 2.2, 1e3
            d = min(d, 2.2)      # cutoff_dist
            v = max(v, 1e-5)
            if not v < 1e3:
                v = 1e3
            D[i, j] = D[j, i] = d
            V[i, j] = V[j, i] = v
        joins, _, _ = bionj_ref.bionj_joins(D, V)
        clusters = [frozenset([k]) for k in range(n)]
        splits = set()
        everything = frozenset(range(n))
        for j in joins:
            i1, i2 = int(j["index1"]), int(j["index2"])
            clusters[i1] = clusters[i1] | clusters[i2]
            del clusters[i2]
            side = clusters[i1]
            splits.add(everything - side if 0 in side else side)
        found.append(splits)
    _, labelled = labelled_splits(parse_labelled(text))
    assert len(labelled) == n - 3
    for side, labels in labelled.items():
        assert set(labels) == {sum(side in s for s in found)}, (sorted(side), labels)
