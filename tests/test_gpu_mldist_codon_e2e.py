"""ML distances of the codon model and of a generator without an eigen form on the device, through the product driver: `pgmsa -a -m
-T -i 0 --dump_dist` with PGM_DEVICE_MLDIST=1 (pgm_mldist_general_kernel) against the same run with the host estimator.

The dumped distance and variance matrices agree within the bound of tests/test_gpu_mldist_general.py (measured there),
and `--stats` of the device run reports every pair as estimated by the device kernel (mldist_device_pairs; without the general
form the 61-state model never reached the device).  Trees are not compared: an exact BioNJ tie may fall the other way.

--batch refuses --dump_dist, so the batch run is checked in two steps: its --stats reports the pairs of all three families as
estimated on the device, and every family's output is the one the device run writes for that family alone, whose matrices are
compared with the host's.  The --custom_model file format holds a symmetric exchangeability matrix, which always has an eigen form;
the amino-acid generator without one is a wag.qmat with its off-diagonal rates perturbed one by one, in a data directory of its
own (PGM_DATA_DIR)."""
import os
import shutil

import numpy as np
import pytest

import batch_util as bu
import gen
import mldist_general_ref as R
from test_gpu_mldist_general import DIST_BOUND, VAR_BOUND

pytestmark = pytest.mark.gpu
OPTS = ["-a", "-m", "-T", "-i", "0"]


def _env(device, data_dir=None):
    env = dict(os.environ)
    env.pop("PGM_DEVICE_MLDIST", None)
    env.pop("PGM_DATA_DIR", None)
    if device:
        env["PGM_DEVICE_MLDIST"] = "1"
    if data_dir:
        env["PGM_DATA_DIR"] = data_dir
    return env


def _solo(opts, fa, tmp_path, device, data_dir=None):
    """One solo run; returns (stdout, --stats record, [(D, V)])."""
    import prographmsa_amd as pg
    dump = os.path.join(str(tmp_path), "%s.%d.dist" % (os.path.basename(fa), device))
    if os.path.exists(dump):
        os.remove(dump)
    r = bu.run(pg.PGMSA_PATH, list(opts) + OPTS + ["--stats", "--dump_dist", dump, fa], _env(device, data_dir))
    return r.stdout, bu.stats_of(r.stderr), R.read_dump(dump)


def _compare(fa, opts, tmp_path, npairs, data_dir=None):
    """host against device on one family; returns the device run's stdout"""
    _, sh, mh = _solo(opts, fa, tmp_path, 0, data_dir)
    out, sd, md = _solo(opts, fa, tmp_path, 1, data_dir)
    assert "mldist_device_pairs" not in sh
    assert sd["mldist_device_pairs"] == npairs and sd["mldist_kernel_ms"] > 0, sd
    assert len(mh) == len(md) == 1
    wd, wv = R.rel_diff(md[0][0], mh[0][0]), R.rel_diff(md[0][1], mh[0][1])
    print("%s: device vs host max rel diff dist %.3e var %.3e, kernel %.3f ms" % (os.path.basename(fa), wd, wv, sd["mldist_kernel_ms"]))
    assert np.count_nonzero(mh[0][0]) == 2 * npairs                  # every pair of the matrix is compared
    assert wd <= DIST_BOUND and wv <= VAR_BOUND, (wd, wv)
    return out


def _codon_family(tmp_path, seed):
    fa = os.path.join(str(tmp_path), "cod%d.fa" % seed)
    with open(fa, "w") as f:
        f.write(gen.fasta(gen.gen_codon(12, 60, seed, sub=0.15)))
    return fa


def test_codon_run(tmp_path):
    _compare(_codon_family(tmp_path, 41), ["--codon"], tmp_path, 66)


def test_codon_batch_run(tmp_path):
    import prographmsa_amd as pg
    fams = [_codon_family(tmp_path, s) for s in (41, 42, 43)]
    solo = [_compare(fa, ["--codon"], tmp_path, 66) for fa in fams]
    outs, stats, _ = bu.run_batch(pg.PGMSA_PATH, fams, ["--codon"] + OPTS, tmp_path, "dev", env=_env(1))
    assert stats["mldist_device_pairs"] == 3 * 66 and stats["mldist_kernel_ms"] > 0, stats
    bu.assert_identical(outs, solo)
    outs_h, stats_h, _ = bu.run_batch(pg.PGMSA_PATH, fams, ["--codon"] + OPTS, tmp_path, "host", env=_env(0))
    assert "mldist_device_pairs" not in stats_h


def test_amino_acid_generator_without_an_eigen_form(tmp_path):
    data = os.path.join(str(tmp_path), "data")
    shutil.copytree(R.DATA, data)
    Q = R.read_qmat(os.path.join(R.DATA, "wag.qmat"))
    rng = np.random.default_rng(9)
    Q = Q * rng.uniform(0.6, 1.4, Q.shape)                           # every rate on its own: no longer reversible
    with open(os.path.join(data, "wag.qmat"), "w") as f:
        f.write("20 20\n" + "\n".join(repr(float(x)) for x in Q.reshape(-1, order="F")) + "\n")
    fa = os.path.join(str(tmp_path), "aa.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta(gen.gen(12, 60, 44, sub=0.15)))
    _compare(fa, [], tmp_path, 66, data_dir=data)
    # (the shipped WAG keeps its eigen form and the 20-state kernel)
    assert _solo([], fa, tmp_path, 1)[1]["mldist_device_pairs"] == 66
