"""The layout of the five scratch slots the four tree-likelihood entries share (csrc/pgm_treelik_plan.h), with the host compiler
alone: tests/native/treelik_plan_test.cpp walks every mode over ncols {1, 2, 15, 17}, ncat {1, 3, 16}, trees of 3, 4 and 8 leaves from
a star to a binary tree, ncand {1, 2, 12}, derivs, anc_post asked and not, dim {1, 3, 64}, and checks every region's size, slot,
alignment and that no two overlap, and that every slot ends with its last region."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prographmsa_amd", "csrc")


def test_regions_of_every_mode_and_shape(tmp_path):
    exe = str(tmp_path / "treelik_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "treelik_plan_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    # plain 2, rates 2 x 3, ancestral 2 x 3, nni 3 x 3 per (dim, tree, ncols); the trees: 2 + 3 + 7 node counts
    assert r.stdout == "%d plans\n" % ((2 + 6 + 6 + 9) * 3 * 12 * 4)


def test_plan_and_check_headers_are_host_only():
    for name in ("pgm_treelik_plan.h", "pgm_treelik_check.h"):
        includes = [ln for ln in open(os.path.join(CSRC, name)).read().splitlines() if ln.startswith("#include")]
        assert includes and not any("_kernels.h" in ln or "hip_runtime" in ln for ln in includes), (name, includes)
