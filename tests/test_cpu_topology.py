"""--topology without a GPU: the oracle driver (host loop bionj_joins_host with the plan of build_topo_plan) against every golden
of tests/golden/topology.json (outputs of the reference binary) byte for byte, its --dump_joins against the independent
statement of tests/topology_ref.py applied to the dumped matrices bit for bit (the plans included), the errors, and --batch with
a topology as a family's fourth field."""
import json
import os
import subprocess

import numpy as np
import pytest

import batch_util as bu
import bionj_ref as B
import gen
import topology_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GOLDEN = json.load(open(os.path.join(GOLD, "topology.json")))
FAMILIES = sorted(set((c["n"], c["L"], c["seed"], c["sub"], c["indel"]) for c in GOLDEN["trees"]))
KINDS = ["own", "swapped", "ladder", "ladder_shuffled", "random", "extra_leaves"]


def write(path, text):
    with open(str(path), "w") as f:
        f.write(text)
    return str(path)


def dump_run(exe, args, d, tag):
    """One driver run with both dumps; returns (stdout, [(D, V)], [(n, joins, final_d)])."""
    dd, dj = os.path.join(str(d), tag + ".dist"), os.path.join(str(d), tag + ".joins")
    r = bu.run(exe, list(args[:-1]) + ["--dump_dist", dd, "--dump_joins", dj, args[-1]])
    return r.stdout, B.read_dist_dump(dd), B.read_joins_dump(dj)


def assert_statement(names, topology, dists, joins):
    """Every dumped join record is the statement's for the dumped matrices and the plan of the topology."""
    plan = T.build_topo_plan(sorted(names), T.parse_newick(topology))
    assert len(plan) == len(names) - 1
    assert len(dists) == len(joins) and len(dists) > 0
    for (D, V), (n, jrec, final_d) in zip(dists, joins):
        assert n == len(names) == D.shape[0] and len(jrec) == n - 3
        assert T.read_plan_joins(jrec) == plan[:n - 3]
        rj, rf, _ = T.bionj_joins_plan(D, V, plan)
        assert B.same_bits(rj, jrec), (rj, jrec)
        assert B.same_bits(rf, final_d), (rf, final_d)


def test_the_fixture_holds_what_the_issue_lists():
    assert len(FAMILIES) == 12 and len(GOLDEN["trees"]) == 12 * 2 * len(KINDS)
    for fam in FAMILIES:
        for flow in ("nw", "angle"):
            assert sorted(c["kind"] for c in GOLDEN["trees"] if (c["n"], c["L"], c["seed"], c["sub"], c["indel"]) == fam and c["flow"] == flow) == sorted(KINDS)
    assert [(c["fasta"], c["tree"]) for c in GOLDEN["fasta"]] == [("c1.fa", None), ("x1.fa", None), ("c1.fa", "c1.tree")]
    assert not any("-m" in c["flags"] or "-M" in c["flags"] for c in GOLDEN["trees"] + GOLDEN["fasta"])


@pytest.mark.parametrize("fam", FAMILIES, ids=["n%d_s%d" % (f[0], f[2]) for f in FAMILIES])
def test_golden_trees(oracle_build, tmp_path, fam):
    """The twelve cases of one family (six topologies, NW and k-mer distances): the reference's newick byte for byte, and the join
    record against the statement."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    n, L, seed, sub, indel = fam
    fa = write(tmp_path / "t.fa", gen.fasta(gen.gen(n, L, seed, sub=sub, indel=indel)))
    names = ["seq%04d" % i for i in range(n)]
    cases = [c for c in GOLDEN["trees"] if (c["n"], c["L"], c["seed"], c["sub"], c["indel"]) == fam]
    for k, c in enumerate(cases):
        tp = write(tmp_path / ("t%d.nwk" % k), c["topology"] + "\n")
        out, dists, joins = dump_run(exe, c["flags"] + ["--topology", tp, fa], tmp_path, "t%d" % k)
        assert out == c["stdout"], (c["kind"], c["flow"])
        assert len(joins) == 1
        assert_statement(names, c["topology"], dists, joins)


@pytest.mark.parametrize("k", range(len(GOLDEN["fasta"])), ids=["c1_default", "x1_default", "c1_tree_i1"])
def test_golden_alignments(oracle_build, tmp_path, k):
    """The full flow: the topology holds for the initial tree (unless -t gives one) and for every re-estimation."""
    c = GOLDEN["fasta"][k]
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    tp = write(tmp_path / "t.nwk", c["topology"] + "\n")
    fa = os.path.join(GOLD, c["fasta"])
    args = c["flags"] + (["-t", os.path.join(GOLD, c["tree"])] if c["tree"] else []) + ["--topology", tp, fa]
    out, dists, joins = dump_run(exe, args, tmp_path, "f")
    assert out == c["stdout"]
    if c["tree"]:   # -t … -i 1: no initial estimate, one pass, one re-estimation
        expected = 1
    else:   # the default two passes: the initial estimate, the one after pass 0, and the one after pass 1 unless that pass's
        # alignment (what `-i 1` ends on) equals the alignment of pass 0 (what `-i 0` ends on), where the loop stops as converged
        ends = [bu.run(exe, c["flags"] + ["-i", str(i), "--topology", tp, fa]).stdout for i in (0, 1)]
        expected = 2 if ends[0] == ends[1] else 3
    assert len(joins) == expected
    names = [l[1:].strip() for l in open(fa) if l.startswith(">")]
    assert_statement(names, c["topology"], dists, joins)


def test_the_two_statements_of_the_sums_and_of_the_joins_agree():
    """topology_ref.column_sum is bionj_ref.column_sums for one column, and the joins with the plan that the criterion itself
    chose are the joins of bionj_ref.bionj_joins."""
    rng = np.random.default_rng(5)
    for dim in (4, 5, 6, 7, 8, 9, 31, 64, 65):
        R = rng.uniform(0.0, 2.0, (dim, dim))
        ref = B.column_sums(R)
        for j in range(dim):
            assert T.column_sum(R[:, j], j).tobytes() == ref[j].tobytes(), (dim, j)
    for kind in ("random", "asym", "tiny", "lambda"):
        for n in (4, 9, 33):
            D, V = B.matrices(kind, n)
            rj, rf, _ = B.bionj_joins(D, V)
            pj, pf, _ = T.bionj_joins_plan(D, V, T.read_plan_joins(rj))
            assert B.same_bits(rj, pj) and B.same_bits(rf, pf), (kind, n)


def test_plan_order_and_pruning():
    names = ["a", "b", "c", "d", "e"]
    # the nodes whose children are all leaves first, in pre-order of the file, then first in, first out
    assert T.build_topo_plan(names, T.parse_newick("(((a:1,b:1):1,c:1):1,(d:1,e:1):1);")) == [(0, 1), (2, 3), (0, 1), (0, 1)]
    assert T.build_topo_plan(names, T.parse_newick("((d:1,e:1):1,((a:1,b:1):1,c:1):1);")) == [(3, 4), (0, 1), (0, 1), (0, 1)]
    # leaves that are no sequence: no join, the other child's cluster moves up
    assert T.build_topo_plan(names, T.parse_newick("(((a:1,x:1):1,(y:1,z:1):1):1,((b:1,c:1):1,(d:1,e:1):1):1);")) == [(1, 2), (2, 3), (1, 2), (0, 1)]
    with pytest.raises(T.TopologyError, match='sequence "c"is missing in given topology'):
        T.build_topo_plan(names, T.parse_newick("((a:1,b:1):1,(d:1,e:1):1);"))


def test_errors(oracle_build, tmp_path):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    fa = write(tmp_path / "t.fa", gen.fasta(gen.gen(6, 80, 3)))
    opts = ["-T", "-i", "0"]
    missing = write(tmp_path / "missing.nwk", "((((seq0000:1,seq0001:1):1,seq0003:1):1,seq0004:1):1,seq0005:1);\n")
    r = bu.run(exe, opts + ["--topology", missing, fa], code=2)
    assert 'sequence "seq0002"is missing in given topology' in r.stderr and r.stdout == ""
    three = write(tmp_path / "three.nwk", "(((seq0000:1,seq0001:1,seq0002:1):1,seq0003:1):1,(seq0004:1,seq0005:1):1);\n")
    r = bu.run(exe, opts + ["--topology", three, fa], code=2)
    assert "node with 3 children" in r.stderr and r.stdout == ""
    one = write(tmp_path / "one.nwk", "((((seq0000:1,seq0001:1):1):1,(seq0002:1,seq0003:1):1):1,(seq0004:1,seq0005:1):1);\n")
    r = bu.run(exe, opts + ["--topology", one, fa], code=2)
    assert "node with 1 children" in r.stderr and r.stdout == ""
    twice = write(tmp_path / "twice.nwk", "((((seq0000:1,seq0001:1):1,seq0002:1):1,(seq0002:1,seq0003:1):1):1,(seq0004:1,seq0005:1):1);\n")
    r = bu.run(exe, opts + ["--topology", twice, fa], code=2)
    assert "more than once" in r.stderr
    r = bu.run(exe, opts + ["--topology", str(tmp_path / "absent.nwk"), fa], code=2)
    assert "cannot open topology file" in r.stderr
    # a valid topology afterwards; with -t and no iteration the topology is not used
    good = write(tmp_path / "good.nwk", T.format_topology(T.ladder(["seq%04d" % i for i in range(6)])) + "\n")
    tree = bu.run(exe, opts + ["--topology", good, fa]).stdout
    assert sorted(T.leaves(T.parse_newick(tree))) == ["seq%04d" % i for i in range(6)]
    given = write(tmp_path / "given.nwk", bu.run(exe, opts + [fa]).stdout)
    assert bu.run(exe, opts + ["-t", given, "--topology", good, fa]).stdout == open(given).read()
    assert "--topology" in subprocess.run([exe, "-h"], capture_output=True, text=True).stderr


@pytest.mark.parametrize("opts", [["--fasta"], ["-T", "-i", "0", "-a"], ["--fasta", "-i", "1"]], ids=["default", "nw_tree", "i1"])
def test_batch_with_fourth_fields(oracle_build, tmp_path, opts):
    """A mixed list (plain, -t, topology, both; a family of three): every output is the solo run's."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    fams = T.topology_families(tmp_path)
    assert sum(1 for _, tree, topo in fams if topo and not tree) >= 2 and sum(1 for _, tree, topo in fams if not topo and not tree) >= 1
    assert sum(1 for _, tree, topo in fams if tree and not topo) >= 1 and sum(1 for _, tree, topo in fams if tree and topo) >= 1
    st = T.batch_against_solo(exe, exe, fams, opts, tmp_path)
    assert st["batch_families"] == len(fams) and st["batch_failed"] == 0


def test_batch_reports_a_family_whose_topology_does_not_fit(oracle_build, tmp_path):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    fams = T.topology_families(tmp_path, sizes=(5, 6, 7))
    bad = write(tmp_path / "bad.topo", "((seq0000:1,seq0001:1):1,(seq0002:1,seq0003:1):1);\n")
    lst = tmp_path / "fams.list"
    outs = [str(tmp_path / ("o%d" % i)) for i in range(3)]
    lst.write_text("".join("%s\t%s\t\t%s\n" % (fa, o, bad if i == 1 else "") for i, ((fa, _, _), o) in enumerate(zip(fams, outs))))
    r = bu.run(exe, ["--batch", str(lst), "--fasta", "--stats"], code=2)
    assert 'sequence "seq0004"is missing in given topology' in r.stderr
    st = bu.stats_of(r.stderr)
    assert st["batch_failed"] == 1 and os.path.exists(outs[0]) and os.path.exists(outs[2]) and not os.path.exists(outs[1])
    bu.assert_identical([outs[0], outs[2]], [bu.run(exe, ["--fasta", fams[i][0]]).stdout for i in (0, 2)])


def test_batch_refusals(oracle_build, tmp_path):
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    fa = os.path.join(GOLD, "c1.fa")
    topo = write(tmp_path / "t.nwk", GOLDEN["fasta"][0]["topology"] + "\n")
    lst = tmp_path / "fams.list"
    lst.write_text("%s\t%s\n" % (fa, tmp_path / "c1.out"))
    r = bu.run(exe, ["--batch", str(lst), "--topology", topo], code=2)
    assert "--batch cannot be combined with --topology" in r.stderr
    lst.write_text("%s\t%s\t\t%s\textra\n" % (fa, tmp_path / "c1.out", topo))
    r = bu.run(exe, ["--batch", str(lst), "--fasta"], code=2)
    assert "found 5 field(s)" in r.stderr and not os.path.exists(str(tmp_path / "c1.out"))
