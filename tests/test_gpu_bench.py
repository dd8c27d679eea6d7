"""The benchmark's command line on the GPU: what a plain run prints and what it leaves to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the records that take runs of their own: measured with --full only
FULL_ONLY = ("roofline_leaf", "roofline_pass", "all_pairs_nw", "all_pairs_nw_1024x600", "progressive_strong", "csprofile", "configs",
             "end_to_end", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` on a small family (8 x 60 aa, the debug size): one result line whose value is
    cells_per_step / ms_per_step, the outputs of the last step under --dump-outputs, and none of the records of --full."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--nseq", "8", "--len", "60",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert (out["unit"], out["higher_is_better"], out["dtype"], out["n_gpus"], out["steps"], out["warmup"]) == ("GCUPS", True, "f32", 1, 3, 1)
    assert out["metric"].startswith("DP cell-updates/sec (GCUPS)")
    assert out["config"]["jobs"] == 7 and out["ms_per_step"] > 0
    # value and ms_per_step are the same clock: both are printed with four decimals
    gcups = out["config"]["cells_per_step"] / (out["ms_per_step"] * 1e-3) / 1e9
    assert abs(out["value"] - gcups) <= gcups * 1e-4 / out["ms_per_step"] + 1e-4
    assert not [k for k in FULL_ONLY if k in out]
    score = np.load(tmp_path / "score.npy")
    assert score.shape == (7,) and np.load(tmp_path / "map_len.npy").sum() == np.load(tmp_path / "map1.npy").size
