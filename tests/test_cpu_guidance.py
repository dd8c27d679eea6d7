"""`--guidance` through the CPU oracle driver (pgmsa_oracle: Backend::msa_agreement's default, the host loop): the refusals, the
seeds, the replicates' guide trees against --bootstrap and against a midpoint rooting restated in Python, every replicate's
alignment against the `-t` run on its dumped tree, both score files against a numpy statement made from the written FASTA files
alone (guidance_ref), a family whose conserved half must score above its indel-rich half, and the host residue map and host counts
on hand-made alignments in a stand-alone program under AddressSanitizer and UBSan (tests/native/guidance_test.cpp)."""
import os
import subprocess

import pytest

import batch_util as bu
import gen
import guidance_ref as G
import test_cpu_bootstrap as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return G.families(tmp_path_factory.mktemp("guidance_fams"))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """{3: ..., 5: ...}: families too small and just large enough"""
    all_fams = bu.aa_families(tmp_path_factory.mktemp("guidance_small"))
    return {n: next(f for f in all_fams if f.endswith("_n%d.fa" % n)) for n in (3, 5)}


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(exe, small, tmp_path):
    fa = small[5]
    out = str(tmp_path / "never.tsv")
    res = str(tmp_path / "never.res")
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    topo = str(tmp_path / "topo.nwk")
    with open(topo, "w") as f:
        f.write(bu.run(exe, ["-T", "-i", "0", fa]).stdout)
    both = ["--guidance", "4", "--guidance_out", out, "--guidance_residues", res, "--guidance_dump", str(tmp_path / "never")]
    cases = [
        (["--guidance", "4", fa], "need each other"),
        (["--guidance_out", out, fa], "need each other"),
        (["--guidance_residues", res, fa], "need --guidance"),
        (["--guidance", "0", "--guidance_out", out, fa], "from 1 to 1000"),
        (["--guidance", "1001", "--guidance_out", out, fa], "from 1 to 1000"),
        (["--guidance", "-2", "--guidance_out", out, fa], "from 1 to 1000"),
        (both + [small[3]], "at least 4 sequences"),
        (both + ["--batch", lst], "--batch cannot be combined with --guidance"),
        (["--guidance", "4", "--batch", lst], "--batch cannot be combined with --guidance"),
        (both + ["-T", fa], "cannot be combined with -T"),
        (both + ["-r", fa], "cannot be combined with -r"),
        (both + ["-rr", fa], "cannot be combined with -r"),
        (both + ["-W", fa], "cannot be combined with -W"),
        (both + ["--topology", topo, fa], "cannot be combined with --topology"),
    ]
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [p for p in os.listdir(str(tmp_path)) if p.startswith("never") or p == "b.out"]
        assert left == [], (args, left)


# ---- seeds, stdout, stats ---------------------------------------------------------------------------------------------
def test_seeds_stdout_and_stats(exe, fams, tmp_path):
    fa, opts = fams["aa"]
    a = G.guidance(exe, fa, tmp_path, "a", 4)
    b = G.guidance(exe, fa, tmp_path, "b", 4)
    c = G.guidance(exe, fa, tmp_path, "c", 4, seed=1)                      # the default seed is 1
    assert a.out == b.out == c.out and a.res == b.res == c.res and a.trees == c.trees and a.alns == c.alns
    others = [G.guidance(exe, fa, tmp_path, "s%d" % k, 4, seed=s) for k, s in enumerate((2, 3, 2 ** 63 + 5))]
    assert any(o.trees != a.trees for o in others) and any(o.out != a.out for o in others)
    assert others[0].out.splitlines()[0] == "# guidance replicates=4 seed=2 sequences=13 columns=%d" % (len(G.read_fasta(a.stdout)["seq0000"]))
    plain = bu.run(exe, ["--fasta", "--stats", fa])
    assert a.stdout == plain.stdout                                         # stdout as without the flags
    st = a.stats
    assert st["guidance_replicates"] == 4 and st["guidance_passes"] == 1 and st["guidance_agreement_calls"] == 1
    assert st["guidance_s"] >= st["guidance_align_s"] > 0 and st["guidance_agreement_s"] > 0
    assert not any(k.startswith("guidance") for k in bu.stats_of(plain.stderr))   # the keys come with the flag only
    # --batch_cells cuts the replicates into groups: more passes, more agreement calls, the same files
    g = G.guidance(exe, fa, tmp_path, "g", 4, opts=["--batch_cells", "1"])
    assert g.stats["guidance_passes"] == 4 and g.stats["guidance_agreement_calls"] == 4
    assert g.out == a.out and g.res == a.res and g.alns == a.alns


# ---- the replicates' guide trees ---------------------------------------------------------------------------------------
def test_replicate_trees_are_the_bootstrap_trees_midpoint_rooted(exe, fams, tmp_path):
    fa, _ = fams["aa"]
    N, seed = 6, 77
    boot = str(tmp_path / "boot.nwk")
    r = G.guidance(exe, fa, tmp_path, "t", N, opts=["--bootstrap", str(N), "--bootstrap_out", boot, "--bootstrap_seed", str(seed)], seed=seed)
    assert r.stats["bootstrap_replicates"] == N                              # (its keys count its own replicates only)
    alone = str(tmp_path / "alone.nwk")
    bu.run(exe, ["--fasta", "--bootstrap", str(N), "--bootstrap_out", alone, "--bootstrap_seed", str(seed), fa])
    assert open(alone).read() == open(boot).read()
    names, labelled = TB.labelled_splits(TB.parse_labelled(open(boot).read()))
    assert len(names) == 13 and len(labelled) == 10
    found = []
    for text in r.trees:
        root = G.parse_newick(text)
        leaf_names, splits = G.splits_of(root)
        assert leaf_names == names and len(splits) == 10                     # a binary tree over all sequences
        found.append(splits)
        # binary at the root, and the root halves the longest leaf-to-leaf path
        assert not isinstance(root, str) and len(root) == 2
        tops = [max(G.leaf_depths(kid).values()) + length for kid, length in root]
        longest = G.longest_path(root)
        assert abs(tops[0] + tops[1] - longest) <= 1e-12 * longest and abs(tops[0] - tops[1]) <= 1e-12 * longest, (tops, longest)
    for side, labels in labelled.items():
        want = sum(frozenset(names[k] for k in side) in s for s in found)
        assert set(labels) == {want}, (sorted(side), labels, want)
    assert any(0 < v[0] < N for v in labelled.values()) or len(set(r.trees)) > 1   # (the resamplings are not all one tree)


# ---- the replicates' alignments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
def test_replicate_alignments_are_the_runs_on_their_trees(exe, fams, tmp_path, kind):
    fa, opts = fams[kind]
    r = G.guidance(exe, fa, tmp_path, kind, 6, opts=opts)
    assert len(set(r.alns)) > 1 or len(set(r.trees)) == 1
    for k in range(6):
        solo = bu.run(exe, ["--fasta"] + opts + ["-t", "%s.%d.nwk" % (r.prefix, k), fa]).stdout
        assert len(solo) > 0 and r.alns[k] == solo, (kind, k)


# ---- the scores --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,extra", [("aa", 6, []), ("aa", 1, []), ("codon", 6, []), ("dna", 5, []), ("repeats", 4, []), ("cs", 4, []),
                                          ("aa", 3, ["--ancestral_seqs"]), ("codon", 3, ["-I"])],
                         ids=["aa_start_column", "aa_N1", "codon", "dna", "repeats", "cs", "aa_ancestral", "codon_input_order"])
def test_scores_equal_the_numpy_statement(exe, fams, tmp_path, kind, n, extra):
    fa, opts = fams[kind]
    seed = 5 if kind == "dna" else 1
    r = G.guidance(exe, fa, tmp_path, "s", n, opts=opts + extra, seed=seed)
    base = G.read_fasta(r.stdout)
    if kind == "aa":   # the family carries start characters on some rows: the written alignment has the re-inserted column
        first = {s: row[0] for s, row in base.items() if not s.startswith("(")}
        assert set(first.values()) == {"M", "-"}
    if extra == ["--ancestral_seqs"]:
        assert any(s.startswith("(") for s in base) and any(s.startswith("(") for s in G.read_fasta(r.alns[0]))
    want_out, want_res = G.expected_files(r.stdout, r.alns, 3 if kind == "codon" else 1, seed)
    assert r.out == want_out
    assert r.res == want_res
    assert "(" not in r.out and "(" not in r.res                            # ancestral rows are left out of the scores


# ---- sanity: a conserved block scores above an indel-rich block --------------------------------------------------------
def two_block_family(n, L, seed):
    """Two concatenated blocks evolved along the same (gen's balanced) tree: few substitutions and no indels, then many indels.
    Returns the sequences and the length of every sequence's first block."""
    calm = gen.gen(n, L, seed, sub=0.03, indel=0.0)
    wild = gen.gen(n, L, seed + 1, sub=0.25, indel=0.12)
    seqs = [("A" + c[1:]) + w for c, w in zip(calm, wild)]
    return seqs, [len(c) for c in calm]


def test_conserved_block_scores_above_indel_block(exe, tmp_path):
    seqs, first = two_block_family(12, 60, 31)
    fa = str(tmp_path / "blocks.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta(seqs))
    r = G.guidance(exe, fa, tmp_path, "blocks", 8)
    base = G.read_fasta(r.stdout)
    names = sorted(base)
    L = len(base[names[0]])
    # a column belongs to a block when all of its residues come from that block of their sequences
    block = []
    seen = [0] * len(names)
    for c in range(L):
        kinds = set()
        for i, s in enumerate(names):
            if base[s][c] != "-":
                kinds.add(0 if seen[i] < first[int(s[3:])] else 1)
                seen[i] += 1
        block.append(kinds.pop() if len(kinds) == 1 else None)
    scores = G.column_scores(r.out)
    mean = []
    for b in (0, 1):
        v = [scores[c + 1] for c in range(L) if block[c] == b and scores[c + 1] is not None]
        assert len(v) >= 20, (b, len(v))
        mean.append(sum(v) / len(v))
    print("mean column score: conserved block %.6f, indel-rich block %.6f" % (mean[0], mean[1]))
    assert mean[0] > mean[1]


# ---- the host residue map and the host counts on hand-made alignments --------------------------------------------------
def test_guidance_native_sanitized(tmp_path):
    exe = str(tmp_path / "guidance_test")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", host, "-o", exe, os.path.join(ROOT, "tests", "native", "guidance_test.cpp"), os.path.join(host, "host_threads.cpp"), os.path.join(host, "guidance.cpp"), os.path.join(host, "phytree.cpp"),
                    os.path.join(host, "alphabet.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
