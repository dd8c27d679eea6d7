"""Root search (-r / -rr; reference src/FindRoot.h, src/GapParsimony.h) through the CPU oracle driver.

The DAG of directed merges the driver runs is checked against an independent statement of the reference's search: for
every branch, the guide tree rerooted on it is written as a newick file and aligned by a plain pass; the plain passes'
alignments are scored by a numpy restatement of GapParsimony.h and the winner is picked as FindRoot.h picks it.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import gen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- GapParsimony.h in numpy -------------------------------------------------------------------------------------
def leaf_blocks(gap_row):
    """The reference's bitset of one row: 64-bit blocks of 32 columns, bit 2c residue, bit 2c+1 gap; the padding loop
    `for (i = length % 32; i < 32; ++i)` sets both bits of the rest of the last block, all of it for a multiple of 32."""
    L = len(gap_row)
    nb = (L + 31) // 32
    blocks = np.zeros(nb, np.uint64)
    for i in range(L):
        blocks[i // 32] |= np.uint64(1) << np.uint64(2 * (i % 32) + int(gap_row[i]))
    for i in range(L % 32, 32):
        blocks[nb - 1] |= np.uint64(3) << np.uint64(2 * i)
    return blocks


HI = np.uint64(0xAAAAAAAAAAAAAAAA)


def _popcount(a):
    return int(sum(bin(int(x)).count("1") for x in a))


def gap_parsimony(gaps, children):
    """gaps: nleaves x ncols bool; children: post-order pairs (ids < nleaves rows, nleaves + k internal node k), root last."""
    nl = gaps.shape[0]
    cons = {i: leaf_blocks(gaps[i]) for i in range(nl)}
    score = 0
    for k, (a, b) in enumerate(children):
        x = cons[a] & cons[b]
        t = ~x
        t = t & (t << np.uint64(1)) & HI
        score += _popcount(t)
        cons[nl + k] = x | t | (t >> np.uint64(1))
    return score


def fitch_columns(gaps, children, ncounted):
    """Plain set-based Fitch on the first `ncounted` columns (a second statement for the bit form)."""
    nl = gaps.shape[0]
    score = 0
    for c in range(ncounted):
        sets = {i: {bool(gaps[i, c])} for i in range(nl)}
        for k, (a, b) in enumerate(children):
            s = sets[a] & sets[b]
            if not s:
                score += 1
                s = sets[a] | sets[b]
            sets[nl + k] = s
    return score


# ---- newick and the unrooted graph of FindRoot.h ------------------------------------------------------------------
def parse_newick(text):
    text = text.strip().rstrip(";")
    pos = 0

    def node():
        nonlocal pos
        n = {"children": [], "name": "", "len": 0.0}
        if text[pos] == "(":
            pos += 1
            while True:
                n["children"].append(node())
                if text[pos] == ",":
                    pos += 1
                    continue
                assert text[pos] == ")"
                pos += 1
                break
        m = re.match(r"[^:,();]*", text[pos:])
        n["name"] = m.group(0)
        pos += len(m.group(0))
        if pos < len(text) and text[pos] == ":":
            m = re.match(r"[^,();]*", text[pos + 1:])
            n["len"] = float(m.group(0))
            pos += 1 + len(m.group(0))
        return n

    return node()


class UGraph:
    """tree2graph (FindRoot.h:176-275): nodes[n] = [edge ids] (slot 0 toward the original root), edges[e] = [n0, n1, len];
    with -t every support is 1."""

    def __init__(self, tree):
        self.nodes, self.edges, self.name = [], [], {}
        if len(tree["children"]) == 2:
            self.edges.append([0, 1, tree["children"][0]["len"] + tree["children"][1]["len"]])
            self.nodes += [[0], [0]]
            self._walk(0, tree["children"][0])
            self._walk(1, tree["children"][1])
        elif len(tree["children"]) == 3:
            self.nodes.append([None, None, None])
            for i, c in enumerate(tree["children"]):
                e, n = len(self.edges), len(self.nodes)
                self.edges.append([0, n, c["len"]])
                self.nodes.append([e])
                self.nodes[0][i] = e
                self._walk(n, c)
        else:
            raise ValueError("multifurcation")

    def _walk(self, cur, t):
        if not t["children"]:
            self.name[cur] = t["name"]
            return
        for c in t["children"]:
            e, n = len(self.edges), len(self.nodes)
            self.edges.append([cur, n, c["len"]])
            self.nodes[cur].append(e)
            self.nodes.append([e])
            self._walk(n, c)

    def other(self, e, n):
        a, b, _ = self.edges[e]
        return b if a == n else a

    def sub_newick(self, n, frm):
        if n in self.name:
            return self.name[n]
        parts = [self.sub_newick(self.other(e, n), e) + ":" + repr(self.edges[e][2]) for e in self.nodes[n] if e != frm]
        return "(" + ",".join(parts) + ")"

    def rerooted(self, e):
        """Point 3-4: the candidate of edge e aligns its two sides at half the length each; a side's children are the
        other two edges in ascending slot order."""
        a, b, L = self.edges[e]
        return "(%s:%r,%s:%r);" % (self.sub_newick(a, e), L / 2, self.sub_newick(b, e), L / 2)

    def topology(self, e, row_of):
        ch = []
        nl = len(row_of)

        def sub(n, frm):
            if n in self.name:
                return row_of[self.name[n]]
            ids = [sub(self.other(x, n), x) for x in self.nodes[n] if x != frm]
            ch.append(tuple(ids))
            return nl + len(ch) - 1

        a, b, _ = self.edges[e]
        ch.append((sub(a, e), sub(b, e)))
        return ch


def read_fasta(text):
    names, rows, cur = [], {}, None
    for ln in text.splitlines():
        if ln.startswith(">"):
            cur = ln[1:].strip()
            names.append(cur)
            rows[cur] = ""
        elif cur is not None:
            rows[cur] += ln.strip()
    return names, rows


def exhaustive_pick(scores):
    best = 0
    for e in range(1, len(scores)):
        if scores[e] < scores[best]:
            best = e
    return best


def hill_climb(g, score_of):
    """FindRoot.h:290-320."""
    best_edge, best_node, best = 0, None, score_of(0)
    while True:
        old_edge, old_node = best_edge, best_node
        for i in range(2):
            n = g.edges[old_edge][i]
            if n == old_node:
                continue
            for e in g.nodes[n]:
                if e == old_edge or e is None:
                    continue
                s = score_of(e)
                if s < best:
                    best_edge, best, best_node = e, s, n
        if best_edge == old_edge:
            return best_edge, best


def run(exe, args, cwd=None):
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr


def score_line(score):
    return "best gap parsimony score: %g" % score   # ostream default: 6 significant digits


def check_root_search(exe, fa, tree_text, tmp_path, extra=()):
    """Runs `exe -r` and `exe -rr` and the independent statement; asserts identical FASTA and score lines."""
    g = UGraph(parse_newick(tree_text))
    tree_file = tmp_path / "orig.tree"
    tree_file.write_text(tree_text + "\n")
    cands = []
    for e in range(len(g.edges)):
        (tmp_path / "e.tree").write_text(g.rerooted(e) + "\n")
        out, _ = run(exe, ["-f", *extra, "-t", str(tmp_path / "e.tree"), fa])
        names, rows = read_fasta(out)
        row_of = {n: i for i, n in enumerate(names)}
        gaps = np.array([[c == "-" for c in rows[n]] for n in names], bool)
        cands.append((rows, gap_parsimony(gaps, g.topology(e, row_of))))
    scores = [s for _, s in cands]
    # the output keeps the order of the unrerooted tree (main.cpp:282-285)
    order = [ln[1:] for ln in run(exe, ["-f", *extra, "-rr", "-t", str(tree_file), fa])[0].splitlines() if ln.startswith(">")]
    for flag, (best, best_score) in (("-r", (exhaustive_pick(scores), min(scores))), ("-rr", hill_climb(g, lambda e: scores[e]))):
        out, err = run(exe, ["-f", *extra, flag, "-t", str(tree_file), fa])
        rows = cands[best][0]
        assert out == "".join(">%s\n%s\n" % (n, rows[n]) for n in order), (flag, best)
        assert score_line(best_score) in err.splitlines(), (flag, err)
    return scores


# ---- tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,expect", [(1, 1), (31, 31), (32, 0), (33, 33), (64, 32), (65, 65)])
def test_gap_parsimony_restatement_lengths(L, expect):
    """Two gapped rows against two ungapped rows: one change per counted column; the last 32 columns of a multiple of 32
    are never counted (the padding quirk)."""
    gaps = np.array([[True] * L, [True] * L, [False] * L, [False] * L])
    assert gap_parsimony(gaps, [(0, 1), (2, 3), (4, 5)]) == expect
    # the same leaves in another rooting: the change sits on the root edge or an inner one, the count is the same
    assert gap_parsimony(gaps, [(0, 2), (4, 1), (5, 3)]) == 2 * expect
    counted = L - 32 if L % 32 == 0 else L
    rng = np.random.default_rng(L)
    for _ in range(4):
        g = rng.random((6, L)) < 0.4
        topo = [(0, 1), (2, 6), (3, 4), (8, 5), (7, 9)]
        assert gap_parsimony(g, topo) == fitch_columns(g, topo, counted)


def test_reroot_flag_parsing(oracle_build, tmp_path):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    fa, tr = os.path.join(GOLD, "x1.fa"), os.path.join(GOLD, "x1.tree")
    a = run(exe, ["-f", "-r", "-r", "-t", tr, fa])
    b = run(exe, ["-f", "-rr", "-t", tr, fa])
    c = run(exe, ["-f", "--reroot", "--reroot", "-t", tr, fa])
    assert a == b == c
    assert run(exe, ["-f", "--reroot", "-t", tr, fa]) == run(exe, ["-f", "-r", "-t", tr, fa])
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert "--reroot" in r.stderr


@pytest.mark.parametrize("flag", ["--ancestral_seqs", "--profile_out"])
def test_reroot_refuses_ancestral_outputs(oracle_build, tmp_path, flag):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    args = [flag] + ([str(tmp_path / "p.txt")] if flag == "--profile_out" else [])
    r = subprocess.run([exe, "-f", "-r", *args, "-t", os.path.join(GOLD, "c1.tree"), os.path.join(GOLD, "c1.fa")], capture_output=True, text=True)
    assert r.returncode == 2 and "-r" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("case", ["c1", "x1", "a1"])
def test_root_search_equals_rerooted_plain_passes(oracle_build, tmp_path, case):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    scores = check_root_search(exe, os.path.join(GOLD, case + ".fa"), open(os.path.join(GOLD, case + ".tree")).read().strip(), tmp_path)
    assert len(scores) == 2 * len(read_fasta(open(os.path.join(GOLD, case + ".fa")).read())[0]) - 3


def test_root_search_two_sequences(oracle_build, tmp_path):
    """One branch: the candidate aligns the two leaves at (a + b) / 2 each, not at a and b."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    (tmp_path / "two.fa").write_text(gen.fasta(gen.gen(2, 80, 7, indel=0.05)))
    check_root_search(exe, str(tmp_path / "two.fa"), "(seq0000:0.3,seq0001:0.05);", tmp_path)


def test_root_search_unrooted_newick(oracle_build, tmp_path):
    """A trifurcating root (an unrooted newick) gets three edges at one node."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    t = "((seq0000:0.151065,seq0001:0.0842293):0.0595943,(seq0002:0.0936846,seq0003:0.0345205):0.0926,((seq0006:0.0823794,seq0007:0.0940911):0.0630846,(seq0004:0.0797032,seq0005:0.0883641):0.040634):0.0723236);"
    assert len(parse_newick(t)["children"]) == 3
    check_root_search(exe, os.path.join(GOLD, "c1.fa"), t, tmp_path)


def test_root_search_with_repeats_and_codons_runs(oracle_build, tmp_path):
    """Flags that combine with -r: tandem repeats (the leaves carry their annotation) and codons."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    seqs, trd = gen.gen_repeat_family(6, 90, 3)
    (tmp_path / "r.fa").write_text(gen.fasta(seqs)); (tmp_path / "r.trd").write_text(trd)
    out, err = run(exe, ["-f", "-r", "-R", "--read_repeats", str(tmp_path / "r.trd"), str(tmp_path / "r.fa")])
    assert out.count(">") == 6 and any(ln.startswith("best gap parsimony score: ") for ln in err.splitlines())
    assert any(ln.startswith("TR indels: ") for ln in err.splitlines())
    out, err = run(exe, ["-f", "-rr", "--codon", "-t", os.path.join(GOLD, "cd1.tree"), os.path.join(GOLD, "cd1.fa")])
    assert out.count(">") == open(os.path.join(GOLD, "cd1.fa")).read().count(">")


def _reroot_family(which, tmp_path):
    if which == "c1":
        return ["-t", os.path.join(GOLD, "c1.tree"), os.path.join(GOLD, "c1.fa")]
    seqs, trd = gen.gen_repeat_family(6, 90, 3)
    (tmp_path / "r.fa").write_text(gen.fasta(seqs)); (tmp_path / "r.trd").write_text(trd)
    return ["-R", "--read_repeats", str(tmp_path / "r.trd"), str(tmp_path / "r.fa")]


@pytest.mark.parametrize("flag", ["-r", "-rr"])
@pytest.mark.parametrize("which", ["c1", "repeats"])
def test_root_search_with_resident_profiles(oracle_build, tmp_path, which, flag):
    """The root search with the profiles kept behind the backend (PGM_ORACLE_RESIDENT=1: leaves without host profiles, built by
    the one-hot upload, repeats attached to them) gives the FASTA, the score line and the TR indels lines of the host-profile run."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    args = ["-f", flag, "--stats"] + _reroot_family(which, tmp_path)
    res = {}
    for resident in (False, True):
        env = {k: v for k, v in os.environ.items() if k != "PGM_ORACLE_RESIDENT"}
        if resident:
            env["PGM_ORACLE_RESIDENT"] = "1"
        r = subprocess.run([exe] + args, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        lines = r.stderr.splitlines()
        stats = [ln for ln in lines if ln.startswith("{")]
        assert len(stats) == 1 and ('"resident": true' in stats[0]) == resident, stats
        score = [ln for ln in lines if ln.startswith("best gap parsimony score: ")]
        assert len(score) == 1
        res[resident] = (r.stdout, score, [ln for ln in lines if ln.startswith("TR indels")])
    assert res[True][0].count(">") == (8 if which == "c1" else 6)
    assert res[True] == res[False]
    if which == "repeats":
        assert res[True][2]
