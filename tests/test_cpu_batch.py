"""`pgmsa --batch LIST`: many families per run, every stage shared by the families of a chunk — through the CPU oracle driver.

The contract: every output file of one `--batch` run is byte for byte what the solo run of the same options writes on stdout for
that family alone, whatever the flow, the chunking and the number of workers.  The `--stats` counts show that the stages were
shared: one run_level per height of the tallest tree of a chunk, not one per height of every tree."""
import os

import pytest

import batch_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return bu.aa_families(tmp_path_factory.mktemp("batch_fams"))


@pytest.fixture(scope="module")
def trees(exe, fams, tmp_path_factory):
    return bu.solo_trees(exe, fams, [], tmp_path_factory.mktemp("batch_trees"))


FLOWS = {
    "fasta_t": (["--fasta"], True),
    "fasta": (["--fasta"], False),
    "fasta_a": (["--fasta", "-a"], False),
    "fasta_a_m": (["--fasta", "-a", "-m"], False),
    "fasta_M_i1": (["--fasta", "-M", "-i", "1"], False),
    "fasta_F": (["--fasta", "-F"], False),
    "T_i0": (["-T", "-i", "0"], False),
    "T": (["-T"], False),
    "ancestral": (["--fasta", "--ancestral_seqs"], False),
    "early_refinement": (["--fasta", "--early_refinement"], False),
    "fasta_I": (["--fasta", "-I"], False),
}


def test_the_family_set(fams):
    sizes = sorted(open(f).read().count(">") for f in fams)
    assert sizes == [2, 2, 3, 3, 5, 5, 8, 8, 13, 13, 24, 24]
    assert any(l.startswith("M") for f in fams for l in open(f).read().splitlines())


@pytest.mark.parametrize("flow", sorted(FLOWS))
def test_batch_equals_solo(exe, fams, trees, tmp_path, flow):
    opts, with_trees = FLOWS[flow]
    t = trees if with_trees else None
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, flow, t)
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts, t))
    assert st["batch_families"] == 12 and st["batch_failed"] == 0 and st["batch_chunks"] == 1


@pytest.mark.parametrize("flow", ["fasta", "fasta_M_i1"])
def test_host_counts_batch_equals_solo(exe, fams, tmp_path, flow):
    """PGM_HOST_COUNTS=1: the pair counts of the re-estimated guide trees come from the host threads, in one pass over the pairs of
    all families (the counting loop the solo run uses), and every file is that of the solo run with the same variable."""
    env = dict(os.environ, PGM_HOST_COUNTS="1")
    opts, _ = FLOWS[flow]
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, "hc_" + flow, env=env)
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts, env=env))
    assert st["batch_families"] == 12 and st["batch_failed"] == 0 and st["batch_chunks"] == 1
    assert st["batch_dist_calls"] == 1   # the cosine call: no pair-count call was made


def test_dna_custom_model(exe, tmp_path):
    fams = bu.dna_families(tmp_path)
    opts = ["--fasta", "--dna", "--custom_model", bu.hky_model(tmp_path)]
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, "dna")
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts))
    assert st["batch_families"] == 4 and st["batch_failed"] == 0


def test_codon_with_trees(exe, tmp_path):
    fams = bu.codon_families(tmp_path)
    trees = bu.solo_trees(exe, fams, ["--codon"], tmp_path)
    opts = ["--fasta", "--codon"]
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, "codon", trees)
    bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts, trees))
    assert st["batch_families"] == 3 and st["batch_failed"] == 0


def test_list_mixing_lines_with_and_without_a_tree(exe, fams, trees, tmp_path):
    """A family with a tree column behaves as under -t (no iterations unless -i is given), the others iterate."""
    mixed = [t if i % 2 == 0 else None for i, t in enumerate(trees)]
    for opts in (["--fasta"], ["--fasta", "-i", "1"]):
        outs, _, _ = bu.run_batch(exe, fams, opts, tmp_path, "mixed%d" % len(opts), mixed)
        bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts, mixed))


def _estimate(fa):
    """(N - 1) x (mean length)^2 over the start-stripped sequences: the driver's estimate before a tree exists."""
    seqs = [l.strip() for l in open(fa).read().splitlines() if l and not l.startswith(">")]
    lens = [len(s) - (1 if s.startswith("M") else 0) for s in seqs]
    mean = sum(lens) / len(lens)
    return (len(lens) - 1) * mean * mean


def _greedy(cells, bound):
    chunks, cur = 0, None
    for c in cells:
        if cur is None or cur + c > bound:
            chunks, cur = chunks + 1, 0.0
        cur += c
    return chunks


def test_chunking_does_not_change_a_byte(exe, fams, tmp_path):
    opts = ["--fasta"]
    solo = bu.solo_outputs(exe, fams, opts)
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, "own", extra=["--batch_cells", "1"])
    bu.assert_identical(outs, solo)
    assert st["batch_chunks"] == 12
    cells = [_estimate(f) for f in fams]
    bound = next(b for b in (sum(cells) / k for k in (2.0, 2.2, 2.4, 2.6, 2.8, 3.0, 3.3)) if _greedy(cells, b) == 3)
    outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, "three", extra=["--batch_cells", repr(bound)])
    bu.assert_identical(outs, solo)
    assert st["batch_chunks"] == 3


def test_levels_are_shared_by_the_families(exe, fams, trees, tmp_path):
    """The -t flow is one forest pass: one run_level — and at most one align-batch call — per height of the tallest tree, where the solo
    runs make one per height of every tree."""
    heights = [bu.tree_height(open(t).read()) for t in trees]
    outs, st, _ = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "levels", trees)
    assert st["batch_chunks"] == 1 and st["batch_passes"] == 1
    assert st["batch_levels"] == max(heights)
    assert 0 < st["batch_align_calls"] <= max(heights) < sum(heights)
    assert st["batch_dist_calls"] == 0


def test_distance_calls_do_not_grow_with_the_families(exe, fams, tmp_path):
    a = bu.run_batch(exe, fams[:4], ["--fasta"], tmp_path, "d4")[1]
    b = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "d12")[1]
    assert a["batch_dist_calls"] == b["batch_dist_calls"] == 3   # the cosine call, and the pair counts of two rounds


REFUSED = [["-o", "x.out"], ["-t", "x.nwk"], ["-r"], ["-rr"], ["-W"], ["-WW"], ["-R"], ["--read_repeats", "x.treks"], ["--profile_out", "x.prof"],
           ["--dump_jobs", "x.jobs"], ["--dump_dist", "x.dist"], ["POSITIONAL"]]


@pytest.mark.parametrize("extra", REFUSED, ids=[e[0] for e in REFUSED])
def test_refused_options(exe, fams, tmp_path, extra):
    extra = [fams[0]] if extra == ["POSITIONAL"] else [os.path.join(str(tmp_path), e) if e.startswith("x.") else e for e in extra]
    outs = [os.path.join(str(tmp_path), "r%02d.out" % i) for i in range(2)]
    lst = os.path.join(str(tmp_path), "r.list")
    bu.write_list(lst, fams[:2], outs)
    r = bu.run(exe, ["--batch", lst, "--fasta"] + extra, code=2)
    msg = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(msg) == 1 and "--batch" in msg[0], r.stderr
    assert os.listdir(str(tmp_path)) == ["r.list"]


def test_malformed_list_line(exe, fams, tmp_path):
    outs = [os.path.join(str(tmp_path), "m%02d.out" % i) for i in range(3)]
    lst = os.path.join(str(tmp_path), "m.list")
    with open(lst, "w") as f:
        f.write("%s\t%s\n%s\n%s\t%s\n" % (fams[0], outs[0], fams[1], fams[2], outs[2]))
    r = bu.run(exe, ["--batch", lst, "--fasta"], code=2)
    assert "line 2" in r.stderr
    assert not any(os.path.exists(o) for o in outs)
    with open(lst, "w") as f:
        f.write("%s\t%s\t%s\textra\n" % (fams[0], outs[0], fams[1]))
    bu.run(exe, ["--batch", lst, "--fasta"], code=2)
    assert not any(os.path.exists(o) for o in outs)


def test_a_failing_family_does_not_stop_the_others(exe, fams, tmp_path):
    bad = os.path.join(str(tmp_path), "gapped.fa")
    lines = open(fams[4]).read().splitlines()
    lines[1] = lines[1][:10] + "-" + lines[1][10:]
    with open(bad, "w") as f:
        f.write("\n".join(lines) + "\n")
    mine = fams[:4] + [bad] + fams[5:]
    outs, st, err = bu.run_batch(exe, mine, ["--fasta"], tmp_path, "fail", code=2)
    lines = [l for l in err.splitlines() if l.startswith("family ")]
    assert len(lines) == 1 and lines[0].startswith("family %s:" % bad) and "gapped" in lines[0], err
    assert st["batch_failed"] == 1 and st["batch_families"] == 12
    assert not os.path.exists(outs[4])
    solo = bu.solo_outputs(exe, fams, ["--fasta"])
    bu.assert_identical(outs[:4] + outs[5:], solo[:4] + solo[5:])
    r = bu.run(exe, ["--fasta", bad], code=2)   # the solo message is the one reported
    assert r.stderr.strip() in lines[0]


def test_a_tree_naming_an_unknown_sequence(exe, fams, trees, tmp_path):
    wrong = list(trees)
    wrong[3] = trees[5]   # (a tree of another family: more leaves than the family has sequences)
    outs, st, err = bu.run_batch(exe, fams, ["--fasta"], tmp_path, "wrongtree", wrong, code=2)
    assert st["batch_failed"] == 1 and not os.path.exists(outs[3])
    assert any(l.startswith("family %s:" % fams[3]) and "unknown sequence name" in l for l in err.splitlines()), err
    solo = bu.solo_outputs(exe, fams, ["--fasta"], trees)
    bu.assert_identical(outs[:3] + outs[4:], solo[:3] + solo[4:])


@pytest.mark.parametrize("resident", [False, True], ids=["host_profiles", "resident"])
def test_two_workers_same_bytes(exe, fams, trees, tmp_path, resident):
    env = dict(os.environ, PGM_FARM_WORKERS="2")
    if resident:
        env["PGM_ORACLE_RESIDENT"] = "1"   # (the oracle backend then checks that no profile is used on a worker that does not hold it)
    for tag, opts, t in (("w2t", ["--fasta"], trees), ("w2", ["--fasta"], None), ("w2a", ["--fasta", "-a"], None)):
        outs, st, _ = bu.run_batch(exe, fams, opts, tmp_path, tag + str(int(resident)), t, env=env)
        bu.assert_identical(outs, bu.solo_outputs(exe, fams, opts, t))
        assert st["farm_level_workers"] == 2 and st["resident_imports"] == 0
