"""DNA on the MI355X: `pgmsa --dna` byte for byte against the CPU oracle driver over every flow, custom models and -F on amino
acids, and the 4-state prep / emission path (a node's profile is one float4) against the oracle and against the padded
20-state path."""
import os
import subprocess

import numpy as np
import pytest

import test_cpu_dna as T
from test_gpu_dims import _kept_and_product

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ORACLE = os.path.join(ROOT, "oracle", "_build", "pgmsa_oracle")


def pgmsa_path():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


def both(args, files=()):
    """stdout and the listed output files of pgmsa and of pgmsa_oracle for the same arguments (file names get a suffix)."""
    outs = []
    for exe, tag in ((pgmsa_path(), "gpu"), (ORACLE, "cpu")):
        a = [x.replace("@", tag) for x in args]
        r = subprocess.run([exe] + a, capture_output=True, text=True)
        assert r.returncode == 0, (exe, r.stderr)
        outs.append((r.stdout, [open(f.replace("@", tag)).read() for f in files]))
    return outs


@pytest.fixture(scope="module")
def families(tmp_path_factory, oracle_build):
    d = tmp_path_factory.mktemp("dna")
    (d / "hky.model").write_text(T.model_text(*T.HKY))
    out = {}
    for name, (n, L, seed) in {"f16": (16, 600, 101), "f64": (64, 1200, 102), "f256": (256, 1500, 103)}.items():
        (d / (name + ".fa")).write_text(T.dna_family(n, L, seed, n_frac=0.003, case=(name == "f16"))[0])
        out[name] = str(d / (name + ".fa"))
    model = str(d / "hky.model")
    # a guide tree with branch lengths for the -t runs: the oracle's own BioNJ tree of the family
    for name in ("f16", "f256"):
        r = subprocess.run([ORACLE, "--dna", "--custom_model", model, "-T", "-i", "0", out[name]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        (d / (name + ".tree")).write_text(r.stdout)
    return d, out, model


FLOWS = {
    "tree": ["-t", "{tree}"],
    "default": [],
    "a": ["-a"],
    "a_m": ["-a", "-m"],
    "M": ["-M"],
    "F": ["-F"],
    "F_C10": ["-F", "-C", "10"],
    "early": ["--early_refinement"],
    "r": ["-r"],
    "rr": ["-rr"],
    "W": ["-W"],
}


@pytest.mark.parametrize("flow", sorted(FLOWS))
def test_dna_flows_identical_to_oracle(families, flow):
    d, fam, model = families
    args = ["--dna", "--custom_model", model, "--fasta"] + [a.format(tree=str(d / "f16.tree")) for a in FLOWS[flow]] + [fam["f16"]]
    (g, _), (c, _) = both(args)
    assert g == c
    assert len(g.split(">")) == 17
    if flow != "tree":   # the newick of the same flow (-T)
        (g, _), (c, _) = both(["-T"] + args)
        assert g == c and g.startswith("(")


def test_dna_ancestral_and_profiles_identical_to_oracle(families, tmp_path):
    d, fam, model = families
    prof = str(tmp_path / "p.@.txt")
    (g, [pg_]), (c, [pc]) = both(["--dna", "--custom_model", model, "--fasta", "--ancestral_seqs", "--profile_out", prof, "-t",
                                  str(d / "f16.tree"), fam["f16"]], files=[prof])
    assert g == c and pg_ == pc
    assert "\nT\t" in pg_ and "\nG\t" in pg_   # (the profile rows are named in TCAG order)


@pytest.mark.parametrize("flow", ["default", "a_m", "F"])
def test_dna_64_identical_to_oracle(families, flow):
    d, fam, model = families
    (g, _), (c, _) = both(["--dna", "--custom_model", model, "--fasta"] + FLOWS[flow] + [fam["f64"]])
    assert g == c


def test_dna_256_identical_to_oracle(families):
    """256 x 1500 nt: the guide tree of the default flow (angle distances, K = 6: 4096 columns per sequence) and one pass on it."""
    d, fam, model = families
    (g, _), (c, _) = both(["--dna", "--custom_model", model, "-T", "-i", "0", fam["f256"]])
    assert g == c == open(str(d / "f256.tree")).read()
    (g, _), (c, _) = both(["--dna", "--custom_model", model, "--fasta", "-t", str(d / "f256.tree"), fam["f256"]])
    assert g == c


@pytest.mark.parametrize("case", ["c1", "c2"])
@pytest.mark.parametrize("flags", [["--custom_model", "{model}"], ["-F"], ["--custom_model", "{model}", "-F", "-C", "50"]], ids=["custom", "F", "custom_F"])
def test_aa_custom_model_and_F_identical_to_oracle(tmp_path, oracle_build, case, flags):
    S, f = T.random_model(20, 5)
    (tmp_path / "aa.model").write_text(T.model_text(S, f))
    args = [x.format(model=str(tmp_path / "aa.model")) for x in flags]
    fa, tree = os.path.join(GOLD, case + ".fa"), os.path.join(GOLD, case + ".tree")
    (g, _), (c, _) = both(args + ["--fasta", "-t", tree, fa])
    assert g == c
    (g, _), (c, _) = both(args + ["--fasta", fa])
    assert g == c


# ---- the 4-state kernels ------------------------------------------------------------------------------------------------
def _mixed_job(seed, dim, L, n2):
    """A sequence graph (one-hot rows, some uniform) against a merged graph with skip edges and profile columns."""
    from prographmsa_amd import jobs as J
    seq = J.sequence_job(seed, L, 10, dim)
    other = J.random_job(seed + 1, 12, n2, dim=dim, skip_frac=0.2)
    seq.g2 = other.g2
    return seq


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_small_dims_bit_exact(ctx, dim):
    """Batches whose largest alphabet is 1-4 (the DP = 4 path): profile rows, one-hot rows, and a sequence graph against a merged
    graph; DP matrices, scores and tracebacks against the oracle, in the kept form and in the product form."""
    from prographmsa_amd import jobs as J
    js = [J.random_job(41000 + 10 * dim + k, n1, n2, dim=dim, skip_frac=0.15) for k, (n1, n2) in enumerate([(130, 97), (517, 129), (66, 65)])]
    js += [J.sequence_job(41100 + 10 * dim + k, L1, L2, dim, unknown_frac=0.05 * k) for k, (L1, L2) in enumerate([(300, 280), (90, 1100), (64, 64)])]
    js.append(_mixed_job(41200 + 10 * dim, dim, 400, 350))
    _kept_and_product(ctx, js)


def test_mixed_4_and_20_takes_the_padded_path(ctx):
    from prographmsa_amd import jobs as J
    js = [J.random_job(42000, 300, 260, dim=4, skip_frac=0.2), J.sequence_job(42001, 400, 380, 4), _mixed_job(42002, 4, 250, 270),
          J.random_job(42003, 200, 210, dim=20, skip_frac=0.1)]
    _kept_and_product(ctx, js)


def test_four_state_S_alone_equals_padded(ctx):
    """The emission scores (and M, X, Y, W) of 4-state jobs are bit-equal whether they run alone (DP = 4) or beside a 20-state
    job (DP = 20: the padded terms are exact zeros)."""
    from prographmsa_amd import jobs as J
    four = [J.random_job(43000, 350, 300, dim=4, skip_frac=0.15), J.sequence_job(43001, 320, 290, 4, unknown_frac=0.05),
            _mixed_job(43002, 4, 300, 280)]
    twenty = J.random_job(43003, 150, 170, dim=20, skip_frac=0.1)
    mats = []
    for js in (four, four + [twenty]):
        b = J.Batch(ctx, js, keep_matrices=True)
        b.run()
        res = b.fetch()
        mats.append([(b.read_matrices(i), res[i]) for i in range(len(four))])
        b.close()
    for (ma, ra), (mb, rb) in zip(*mats):
        for x, y in zip(ma, mb):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.float32(ra["score"]).view(np.uint32) == np.float32(rb["score"]).view(np.uint32)
        assert np.array_equal(ra["map1"], rb["map1"]) and np.array_equal(ra["map2"], rb["map2"])
