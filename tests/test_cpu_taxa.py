"""`--bootstrap_taxa`, `--bootstrap_taxa_cutoff` and `--bootstrap_taxa_edges` through the CPU oracle driver (pgmsa_oracle:
Backend::transfer_taxa's default, the host loop): the refusals, every other output unchanged, both files against the texts
tests/taxa_ref.py makes from the `--bootstrap_out` tree and the dumped trees alone (byte for byte) at cutoffs 0, 0.3 and 0.99,
seeds, the route switches, and transfer_taxa_host / taxa_support on hand-written trees in a stand-alone program under
AddressSanitizer and UBSan (tests/native/taxa_test.cpp)."""
import os
import subprocess
from types import SimpleNamespace

import pytest

import batch_util as bu
import taxa_ref as X
import test_cpu_transfer as TC
import transfer_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
KEYS = ("bootstrap_taxa_s", "bootstrap_taxa_calls", "bootstrap_taxa_kernel_ms")


def run_taxa(exe, fa, d, tag, opts=(), cutoff=None, seed=None, env=None, taxa=True, edges=True, tbe=True, trees=True, n=N):
    """One driver run with --bootstrap and the flags asked for; the five files (None where not written), stdout, the --stats record."""
    p = {k: os.path.join(str(d), "%s.%s" % (tag, k)) for k in ("out", "tbe", "trees", "taxa", "edges")}
    args = ["--fasta", "--stats", "--bootstrap", str(n), "--bootstrap_out", p["out"]] + (["--bootstrap_seed", str(seed)] if seed is not None else [])
    args += (["--bootstrap_tbe", p["tbe"]] if tbe else []) + (["--bootstrap_trees", p["trees"]] if trees else [])
    args += (["--bootstrap_taxa", p["taxa"]] if taxa else []) + (["--bootstrap_taxa_edges", p["edges"]] if edges else [])
    args += ["--bootstrap_taxa_cutoff", cutoff] if cutoff is not None else []
    r = bu.run(exe, args + list(opts) + [fa], env)
    read = lambda k: open(p[k]).read() if os.path.exists(p[k]) else None
    return SimpleNamespace(stdout=r.stdout, stats=bu.stats_of(r.stderr), **{k: read(k) for k in p})


def check_against_python(run, n_taxa, cutoff="0.3", n=N):
    """Both files are the texts taxa_ref makes from the --bootstrap_out line and the dumped trees; returns taxa_ref's detail."""
    lines = run.trees.splitlines()
    assert len(lines) == n
    want, want_edges, detail = X.taxa_texts(run.out, lines, cutoff)
    assert run.taxa == want
    assert run.edges == want_edges
    rows = run.taxa.splitlines()
    assert len(rows) == 2 + n_taxa and rows[1] == "taxon\tmoved\tscore"
    assert [r.split("\t")[0] for r in rows[2:]] == sorted(T.leaves(T.parse(run.out)))
    labels, _ = T.labels_of(run.out)
    assert len(run.edges.splitlines()) - 1 >= len(labels) > 0   # a row per labelled node (labels_of keys by set: two nodes may share one)
    return detail


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return TC.families(tmp_path_factory.mktemp("taxa_fams"))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(exe, fams, tmp_path):
    fa = fams[5]
    out, taxa, edges = (str(tmp_path / ("never." + k)) for k in ("out", "taxa", "edges"))
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    topo = str(tmp_path / "topo.nwk")
    with open(topo, "w") as f:
        f.write(bu.run(exe, ["-T", "-i", "0", fa]).stdout)
    boot = ["--bootstrap", "4", "--bootstrap_out", out]
    full = boot + ["--bootstrap_taxa", taxa, "--bootstrap_taxa_edges", edges, "--bootstrap_taxa_cutoff", "0.5"]
    cases = [
        (["--bootstrap_taxa", taxa, fa], "need --bootstrap"),                      # a new flag without --bootstrap
        (["--bootstrap_taxa_edges", edges, fa], "need --bootstrap"),
        (["--bootstrap_taxa_cutoff", "0.5", fa], "need --bootstrap"),
        (["--bootstrap", "4", "--bootstrap_taxa", taxa, fa], "need each other"),   # ... without --bootstrap_out
        (["--bootstrap_out", out, "--bootstrap_taxa", taxa, fa], "need each other"),
        (["--bootstrap", "0", "--bootstrap_out", out, "--bootstrap_taxa", taxa, fa], "from 1 to 1000"),
        (boot + ["--bootstrap_taxa_edges", edges, fa], "need --bootstrap_taxa"),   # the two that need --bootstrap_taxa
        (boot + ["--bootstrap_taxa_cutoff", "0.5", fa], "need --bootstrap_taxa"),
        (full + [fams[3]], "at least 4 sequences"),
        (full + ["--batch", lst], "--batch cannot be combined with --bootstrap"),
        (["--bootstrap_taxa", taxa, "--batch", lst], "--batch cannot be combined with --bootstrap"),
        (["--bootstrap_taxa_edges", edges, "--batch", lst], "--batch cannot be combined with --bootstrap"),
        (["--bootstrap_taxa_cutoff", "0.5", "--batch", lst], "--batch cannot be combined with --bootstrap"),
        (full + ["-W", fa], "cannot be combined with -W"),
        (full + ["-r", fa], "cannot be combined with -r"),
        (full + ["-rr", fa], "cannot be combined with -r"),
        (full + ["--topology", topo, fa], "cannot be combined with --topology"),
    ]
    for bad in ("1", "1.0", "1.5", "-0.1", "-1", "nan", "NaN", "-nan", "inf", "-inf", "abc", "", "0.3x", "1e0"):   # the cutoff: 0 <= X < 1 and nothing else
        cases.append((boot + ["--bootstrap_taxa", taxa, "--bootstrap_taxa_cutoff", bad, fa], "0 <= X < 1"))
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [p for p in os.listdir(str(tmp_path)) if p.startswith("never") or p == "b.out"]
        assert left == [], (args, left)


# ---- what does not change, the stats ----------------------------------------------------------------------------------
def test_other_outputs_unchanged_and_stats(exe, fams, tmp_path):
    for n in (5, 24):
        plain = run_taxa(exe, fams[n], tmp_path, "plain%d" % n, taxa=False, edges=False)
        full = run_taxa(exe, fams[n], tmp_path, "full%d" % n)
        alone = run_taxa(exe, fams[n], tmp_path, "alone%d" % n, edges=False, tbe=False, trees=False)   # independent of --bootstrap_tbe
        bare = run_taxa(exe, fams[n], tmp_path, "bare%d" % n, taxa=False, edges=False, tbe=False, trees=False)
        assert plain.taxa is None and plain.edges is None and alone.edges is None and alone.tbe is None and alone.trees is None
        assert full.out == plain.out == alone.out == bare.out and len(plain.out) > 0
        assert full.tbe == plain.tbe and full.trees == plain.trees and len(plain.tbe) > 0
        assert full.stdout == plain.stdout == alone.stdout == bare.stdout == bu.run(exe, ["--fasta", fams[n]]).stdout
        assert full.taxa == alone.taxa
        assert not any(k in plain.stats for k in KEYS) and not any(k in bare.stats for k in KEYS)     # the keys come with the flag only
        for r in (full, alone):
            st = r.stats
            assert st["bootstrap_taxa_calls"] == 1 and st["bootstrap_taxa_s"] > 0 and st["bootstrap_taxa_kernel_ms"] == 0   # (the host loop has no kernel)
            assert st["bootstrap_replicates"] == N and st["bootstrap_s"] >= st["bootstrap_taxa_s"]
        assert "bootstrap_tbe_s" in full.stats and "bootstrap_tbe_s" not in alone.stats
        explicit = run_taxa(exe, fams[n], tmp_path, "explicit%d" % n, cutoff="0.3")                   # the default cutoff is 0.3
        assert (explicit.taxa, explicit.edges) == (full.taxa, full.edges)
        assert full.taxa.startswith("# replicates %d cutoff 0.3 edges " % N)


# ---- the two files ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 13, 24, 70])
@pytest.mark.parametrize("opts", [[], ["-m"]], ids=["default", "m"])
def test_files_equal_the_python_statement(exe, fams, tmp_path, n, opts):
    """Byte for byte at cutoffs 0, 0.3 and 0.99.  The small families have no counted pair with phi > 0 at 0.3 (format and K only);
    the 70-taxon family must have them, and at 0.99 ties between sets that move different taxa, so that nothing passes on zeros."""
    detail = {}
    for cutoff in ("0", "0.3", "0.99"):
        r = run_taxa(exe, fams[n], tmp_path, "t" + cutoff, ["-i", "0"] + opts, cutoff=cutoff, tbe=False)
        detail[cutoff] = check_against_python(r, n, cutoff)
        assert r.taxa.startswith("# replicates %d cutoff %s edges " % (N, cutoff))
    assert all(f == 0 for _, _, f, _ in detail["0"]["pairs"]) and sum(detail["0"]["moved"]) == 0      # thr = 0: only the edges a replicate has
    assert 0 < detail["0"]["K"] <= detail["0.3"]["K"] <= detail["0.99"]["K"]
    if n == 70:
        positive = {c: [p for p in detail[c]["pairs"] if p[2] > 0] for c in ("0.3", "0.99")}
        assert len(positive["0.3"]) > 0 and len(positive["0.99"]) > 0
        assert sum(1 for v in detail["0.3"]["moved"] if v > 0) > 0
        assert sum(1 for _, _, _, ts in positive["0.99"] if len(set(ts)) > 1) > 0                     # minimising sets with different T


def test_only_tree_seeds_and_switches(exe, fams, tmp_path):
    """-T prints what it prints without the flags; the same seed gives the same files, the default seed is 1, another seed other
    trees, each consistent; the route switches give the same bytes."""
    fa = fams[70]
    a = run_taxa(exe, fa, tmp_path, "a", ["-T", "-i", "0"], cutoff="0.99")
    assert a.stdout == bu.run(exe, ["-T", "-i", "0", fa]).stdout
    b = run_taxa(exe, fa, tmp_path, "b", ["-T", "-i", "0"], cutoff="0.99", seed=1)
    assert (a.out, a.trees, a.taxa, a.edges) == (b.out, b.trees, b.taxa, b.edges)
    assert sum(check_against_python(a, 70, "0.99")["moved"]) > 0
    others = [run_taxa(exe, fa, tmp_path, "s%d" % s, ["-T", "-i", "0"], cutoff="0.99", seed=s) for s in (2, 3)]
    for o in others:
        check_against_python(o, 70, "0.99")
        assert o.trees != a.trees
    assert any(o.taxa != a.taxa for o in others) and any(o.edges != a.edges for o in others)
    for switch in ("PGM_HOST_TRANSFER", "PGM_DEVICE_TRANSFER"):   # (this driver's backend has the default body: the host loop either way)
        h = run_taxa(exe, fa, tmp_path, switch, ["-T", "-i", "0"], cutoff="0.99", env=dict(os.environ, **{switch: "1"}))
        assert (h.out, h.tbe, h.trees, h.taxa, h.edges) == (a.out, a.tbe, a.trees, a.taxa, a.edges) and switch in h.stats["switches"]


# ---- the host loop and the sums on hand-written trees -------------------------------------------------------------------
def test_taxa_native_sanitized(tmp_path):
    exe = str(tmp_path / "taxa_test")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    # (-fno-sanitize=vptr: taxa_support calls Backend::transfer_taxa through a pointer, and the check wants Backend's type
    #  information, which lives with the drivers' backends)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize=vptr",
                    "-fno-sanitize-recover=undefined", "-I", host, "-o", exe, os.path.join(ROOT, "tests", "native", "taxa_test.cpp"), os.path.join(host, "host_threads.cpp"), os.path.join(host, "transfer.cpp"),
                    os.path.join(host, "phytree.cpp"), os.path.join(host, "alphabet.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
