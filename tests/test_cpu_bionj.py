"""BioNJ's join record without a GPU: the oracle driver's `-T -i 0 [-a] --dump_dist --dump_joins` (the host loop
bionj_joins_host: the oracle backend has no bionj_multi) against the numpy statement of tests/bionj_ref.py applied to the dumped
matrices, bit for bit.  This is what pins the numpy statement that tests/test_gpu_bionj.py holds the kernels to; the newicks of
the dump runs are those of the goldens (outputs of the reference binary)."""
import json
import os
import subprocess

import numpy as np
import pytest

import bionj_ref as B
import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NW_TREES = json.load(open(os.path.join(GOLD, "nw_trees.json")))


def dump_run(exe, opts, fa, d, tag, env=None):
    """One driver run with both dumps; returns (stdout, [(D, V)], [(n, joins, final_d)])."""
    dd, dj = os.path.join(str(d), tag + ".dist"), os.path.join(str(d), tag + ".joins")
    r = subprocess.run([exe] + list(opts) + ["--dump_dist", dd, "--dump_joins", dj, str(fa)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, B.read_dist_dump(dd), B.read_joins_dump(dj)


def assert_statement(dists, joins):
    assert len(dists) == len(joins) and len(dists) > 0
    for (D, V), (n, jrec, final_d) in zip(dists, joins):
        assert n == D.shape[0] and len(jrec) == n - 3
        rj, rf, _ = B.bionj_joins(D, V)
        assert np.array_equal(rj["index1"], jrec["index1"]) and np.array_equal(rj["index2"], jrec["index2"]), (rj, jrec)
        assert B.same_bits(rj, jrec), (rj, jrec)
        assert B.same_bits(rf, final_d), (rf, final_d)


@pytest.mark.parametrize("k", range(len(NW_TREES)), ids=["n%d_s%d" % (c["n"], c["seed"]) for c in NW_TREES])
@pytest.mark.parametrize("nw", [False, True], ids=["angle", "nw"])
def test_statement_on_the_golden_families(oracle_build, tmp_path, k, nw):
    c = NW_TREES[k]
    fa = tmp_path / "t.fa"
    fa.write_text(gen.fasta(gen.gen(c["n"], c["L"], c["seed"], sub=c["sub"], indel=c["indel"])))
    out, dists, joins = dump_run(os.path.join(oracle_build, "pgmsa_oracle"), ["-T", "-i", "0"] + (["-a"] if nw else []), fa, tmp_path, "t")
    assert len(dists) == 1
    assert_statement(dists, joins)
    if nw:
        assert out == c["tree"]


@pytest.mark.parametrize("case,opts,golden", [("c1.fa", ["-a"], "c1.nw_p.tree"), ("c1.fa", [], None), ("c2.fa", [], "c2.tree"), ("c2.fa", ["-a"], None)],
                         ids=["c1_nw", "c1_angle", "c2_angle", "c2_nw"])
def test_statement_on_c1_c2(oracle_build, tmp_path, case, opts, golden):
    out, dists, joins = dump_run(os.path.join(oracle_build, "pgmsa_oracle"), ["-T", "-i", "0"] + opts, os.path.join(GOLD, case), tmp_path, "c")
    assert_statement(dists, joins)
    if golden:
        assert out == open(os.path.join(GOLD, golden)).read()


def test_dump_joins_of_the_default_flow_and_small_families(oracle_build, tmp_path):
    """The default flow re-estimates the guide tree from the alignment (at most three trees; it stops when the alignment no longer
    changes): one record per tree.  A family of three has no join and final_d is its matrix."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    _, dists, joins = dump_run(exe, ["--fasta"], os.path.join(GOLD, "c1.fa"), tmp_path, "flow")
    assert 2 <= len(joins) <= 3
    assert_statement(dists, joins)
    fa = tmp_path / "three.fa"
    fa.write_text(gen.fasta(gen.gen(3, 80, 5)))
    _, dists, joins = dump_run(exe, ["-T", "-i", "0"], fa, tmp_path, "three")
    (D, V), = dists
    (n, jrec, final_d), = joins
    assert n == 3 and len(jrec) == 0
    off = ~np.eye(3, dtype=bool)
    assert B.same_bits(final_d[off], D[off]) and not final_d.diagonal().any()


def test_dump_joins_is_refused_with_batch(oracle_build, tmp_path):
    lst = tmp_path / "fams.list"
    lst.write_text("%s\t%s\n" % (os.path.join(GOLD, "c1.fa"), tmp_path / "c1.out"))
    r = subprocess.run([os.path.join(oracle_build, "pgmsa_oracle"), "--batch", str(lst), "--dump_joins", str(tmp_path / "j.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--dump_joins" in r.stderr, r.stderr


def test_stats_report_the_host_path(oracle_build, tmp_path):
    r = subprocess.run([os.path.join(oracle_build, "pgmsa_oracle"), "-T", "-i", "0", "--stats", os.path.join(GOLD, "c1.fa")], capture_output=True, text=True,
                       env=dict(os.environ, PGM_DEVICE_BIONJ="1"), timeout=300)
    assert r.returncode == 0, r.stderr
    st = json.loads([l for l in r.stderr.splitlines() if l.startswith("{")][0])
    assert st["bionj_device_calls"] == 0 and st["bionj_launches"] == 0 and st["bionj_s"] > 0
    assert "PGM_DEVICE_BIONJ" in st["switches"]
