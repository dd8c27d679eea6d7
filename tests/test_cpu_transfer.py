"""`--bootstrap_tbe` and `--bootstrap_trees` through the CPU oracle driver (pgmsa_oracle: Backend::transfer_min's default, the host
loop): the refusals, `--bootstrap_out` and stdout unchanged, the dumped replicate trees, the TBE file against the text
tests/transfer_ref.py makes from the `--bootstrap_out` tree and the dumped trees alone (byte for byte), the classical count as the
number of zero transfer indices, seeds, the route switches, and transfer_min_host / transfer_support on hand-written trees in a
stand-alone program under AddressSanitizer and UBSan (tests/native/transfer_test.cpp)."""
import os
import subprocess
from types import SimpleNamespace

import pytest

import batch_util as bu
import gen
import transfer_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8


def families(d):
    """{taxa: FASTA path} for 3, 5, 13, 24 and 70 taxa; the last needs two words per leaf set."""
    all_fams = bu.aa_families(d)
    fams = {n: next(f for f in all_fams if f.endswith("_n%d.fa" % n)) for n in (3, 5, 13, 24)}
    seqs = [("A" + s[1:]) if s[0] == "M" else s for s in gen.gen(70, 60, 4242, sub=0.1)]
    fams[70] = os.path.join(str(d), "fam_n70.fa")
    with open(fams[70], "w") as f:
        f.write(gen.fasta(seqs))
    return fams


def run_tbe(exe, fa, d, tag, opts=(), seed=None, env=None, tbe=True, trees=True, n=N):
    """One driver run with --bootstrap and the new flags; the three files, stdout and the --stats record."""
    p = {k: os.path.join(str(d), "%s.%s" % (tag, k)) for k in ("out", "tbe", "trees")}
    args = ["--fasta", "--stats", "--bootstrap", str(n), "--bootstrap_out", p["out"]] + (["--bootstrap_seed", str(seed)] if seed is not None else [])
    args += (["--bootstrap_tbe", p["tbe"]] if tbe else []) + (["--bootstrap_trees", p["trees"]] if trees else [])
    r = bu.run(exe, args + list(opts) + [fa], env)
    read = lambda k: open(p[k]).read() if os.path.exists(p[k]) else None
    return SimpleNamespace(out=read("out"), tbe=read("tbe"), trees=read("trees"), stdout=r.stdout, stats=bu.stats_of(r.stderr))


def check_against_python(run, n_taxa, n=N):
    """The TBE file is the text transfer_ref makes from the other two files; per labelled edge the classical count is the number
    of replicates with transfer index 0, and TBE >= count / N."""
    lines = run.trees.splitlines()
    assert len(lines) == n and run.trees.endswith("\n")
    want, detail = T.tbe_text(run.out, lines)
    assert run.tbe == want
    counts, names = T.labels_of(run.out)
    printed, _ = T.labels_of(run.tbe)
    assert len(names) == n_taxa and set(counts) == set(printed) == set(detail) and len(detail) >= n_taxa - 3
    for s, (S, p, row) in detail.items():
        count = int(counts[s])
        assert count == sum(1 for v in row if v == 0), (bin(s), count, row)
        assert all(0 <= v <= p - 1 for v in row)
        assert (n * (p - 1) - S) * n >= count * n * (p - 1)                  # TBE >= count / N, in integers
        assert float(printed[s]) >= count / n - 0.5e-6                       # ... and as printed (%.6f rounds by at most 0.5e-6)
    return detail


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return families(tmp_path_factory.mktemp("transfer_fams"))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(exe, fams, tmp_path):
    fa = fams[5]
    out, tbe, trees = (str(tmp_path / ("never." + k)) for k in ("out", "tbe", "trees"))
    lst = str(tmp_path / "b.list")
    bu.write_list(lst, [fa], [str(tmp_path / "b.out")])
    topo = str(tmp_path / "topo.nwk")
    with open(topo, "w") as f:
        f.write(bu.run(exe, ["-T", "-i", "0", fa]).stdout)
    full = ["--bootstrap", "4", "--bootstrap_out", out, "--bootstrap_tbe", tbe, "--bootstrap_trees", trees]
    cases = [
        (["--bootstrap_tbe", tbe, fa], "need --bootstrap"),                   # a new flag without --bootstrap
        (["--bootstrap_trees", trees, fa], "need --bootstrap"),
        (["--bootstrap_tbe", tbe, "--bootstrap_trees", trees, fa], "need --bootstrap"),
        (["--bootstrap", "4", "--bootstrap_tbe", tbe, fa], "need each other"),  # ... without --bootstrap_out
        (["--bootstrap_out", out, "--bootstrap_trees", trees, fa], "need each other"),
        (["--bootstrap", "0", "--bootstrap_out", out, "--bootstrap_tbe", tbe, fa], "from 1 to 1000"),
        (full + [fams[3]], "at least 4 sequences"),
        (full + ["--batch", lst], "--batch cannot be combined with --bootstrap"),
        (["--bootstrap_tbe", tbe, "--batch", lst], "--batch cannot be combined with --bootstrap"),
        (["--bootstrap_trees", trees, "--batch", lst], "--batch cannot be combined with --bootstrap"),
        (full + ["-W", fa], "cannot be combined with -W"),
        (full + ["-r", fa], "cannot be combined with -r"),
        (full + ["-rr", fa], "cannot be combined with -r"),
        (full + ["--topology", topo, fa], "cannot be combined with --topology"),
    ]
    for args, message in cases:
        r = bu.run(exe, ["--fasta"] + args, code=2)
        assert r.stderr.startswith("ERROR:") and message in r.stderr and r.stdout == "", (args, r.stderr)
        left = [p for p in os.listdir(str(tmp_path)) if p.startswith("never") or p == "b.out"]
        assert left == [], (args, left)


# ---- what does not change, the dumped trees, the stats ----------------------------------------------------------------
def test_bootstrap_out_stdout_and_stats(exe, fams, tmp_path):
    for n in (5, 24):
        plain = run_tbe(exe, fams[n], tmp_path, "plain%d" % n, tbe=False, trees=False)
        full = run_tbe(exe, fams[n], tmp_path, "full%d" % n)
        only_trees = run_tbe(exe, fams[n], tmp_path, "trees%d" % n, tbe=False)
        assert plain.tbe is None and plain.trees is None and only_trees.tbe is None
        assert full.out == plain.out == only_trees.out and len(plain.out) > 0        # --bootstrap_out byte for byte
        assert full.stdout == plain.stdout == bu.run(exe, ["--fasta", fams[n]]).stdout
        assert full.trees == only_trees.trees
        lines = full.trees.splitlines()
        names = sorted(T.leaves(T.parse(full.out)))
        assert len(lines) == N and len(names) == n
        for line in lines:
            assert line.endswith(";") and sorted(T.leaves(T.parse(line))) == names
        assert full.tbe.endswith(";\n") and full.tbe.count("\n") == 1
        keys = ("bootstrap_tbe_s", "bootstrap_transfer_calls", "bootstrap_transfer_kernel_ms")
        assert not any(k in plain.stats for k in keys) and not any(k in only_trees.stats for k in keys)   # the keys come with the flag only
        st = full.stats
        assert st["bootstrap_transfer_calls"] == 1 and st["bootstrap_tbe_s"] > 0 and st["bootstrap_transfer_kernel_ms"] == 0   # (the host loop has no kernel)
        assert st["bootstrap_replicates"] == N and st["bootstrap_s"] >= st["bootstrap_tbe_s"]


# ---- the TBE file -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 13, 24, 70])
@pytest.mark.parametrize("opts", [[], ["-m"]], ids=["default", "m"])
def test_tbe_file_equals_the_python_statement(exe, fams, tmp_path, n, opts):
    r = run_tbe(exe, fams[n], tmp_path, "t", ["-i", "0"] + opts)
    detail = check_against_python(r, n)
    if n >= 24:   # (the resamplings of these families are not all one tree: some edge is neither certain nor lost)
        assert any(0 < S < N * (p - 1) for S, p, _ in detail.values())


def test_only_tree_seeds_and_switches(exe, fams, tmp_path):
    """-T prints what it prints without the flags; the same seed gives the same three files, the default seed is 1, another seed
    other trees and with them other files, each consistent; the route switches give the same bytes."""
    fa = fams[24]
    a = run_tbe(exe, fa, tmp_path, "a", ["-T"])
    assert a.stdout == bu.run(exe, ["-T", fa]).stdout
    b = run_tbe(exe, fa, tmp_path, "b", ["-T"])
    c = run_tbe(exe, fa, tmp_path, "c", ["-T"], seed=1)
    assert (a.out, a.tbe, a.trees) == (b.out, b.tbe, b.trees) == (c.out, c.tbe, c.trees)
    check_against_python(a, 24)
    others = [run_tbe(exe, fa, tmp_path, "s%d" % s, ["-T"], seed=s) for s in (2, 3)]
    for o in others:
        check_against_python(o, 24)
        assert o.trees != a.trees
    assert any(o.tbe != a.tbe for o in others) and any(o.out != a.out for o in others)
    for switch in ("PGM_HOST_TRANSFER", "PGM_DEVICE_TRANSFER"):   # (this driver's backend has the default body: the host loop either way)
        h = run_tbe(exe, fa, tmp_path, switch, ["-T"], env=dict(os.environ, **{switch: "1"}))
        assert (h.out, h.tbe, h.trees) == (a.out, a.tbe, a.trees) and switch in h.stats["switches"]


# ---- the host loop and the support on hand-written trees ---------------------------------------------------------------
def test_transfer_native_sanitized(tmp_path):
    exe = str(tmp_path / "transfer_test")
    host = os.path.join(ROOT, "prographmsa_amd", "host")
    # (-fno-sanitize=vptr: transfer_support calls Backend::transfer_min through a pointer, and the check wants Backend's type
    #  information, which lives with the drivers' backends)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize=vptr",
                    "-fno-sanitize-recover=undefined", "-I", host, "-o", exe, os.path.join(ROOT, "tests", "native", "transfer_test.cpp"), os.path.join(host, "host_threads.cpp"), os.path.join(host, "transfer.cpp"),
                    os.path.join(host, "phytree.cpp"), os.path.join(host, "alphabet.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
