"""Goldens of the weighted least-squares guide-tree refinement (-W / -WW; reference src/LeastSquares.cpp, src/NNLS.h).

Usage: python make_golden_wls.py [path/to/ProGraphMSA_64]  ->  wls.json

Trees come from NW distances (-a): their unrefined BioNJ trees already match the reference (nw_trees.json), so these
cases pin the refinement itself.  The FASTA cases add -m (ML distances) and the full flow: the refined supports feed the
progressive alignment, and every -i re-estimation is refined too.  One family holds duplicate sequences: zero distances
make exact ties between the quartet topologies."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen  # noqa: E402

BIN = sys.argv[1] if len(sys.argv) > 1 else "ProGraphMSA_64"

# (taxa, length, seed, substitution rate, indel rate, duplicated sequences)
TREE_CASES = [
    (4, 120, 4101, 0.1, 0.01, 0), (5, 250, 585126, 0.05, 0.005, 0), (7, 120, 59769, 0.1, 0.005, 0),
    (9, 60, 815905, 0.2, 0.005, 0), (12, 100, 1212, 0.1, 0.01, 3), (13, 120, 133400, 0.2, 0.02, 0),
    (16, 120, 653397, 0.2, 0.005, 0), (21, 120, 295589, 0.05, 0.02, 0), (30, 60, 7, 0.1, 0.02, 0),
    (33, 80, 3303, 0.15, 0.01, 0), (64, 100, 6464, 0.1, 0.01, 0), (128, 80, 12828, 0.1, 0.01, 0),
]
FASTA_CASES = [(8, 100, 808, 0.1, 0.01, 0), (12, 100, 1212, 0.1, 0.01, 3), (20, 80, 2020, 0.15, 0.02, 0)]


def family(n, L, seed, sub, indel, dups):
    """gen.gen's family; with dups > 0 the first `dups` sequences appear a second time under names of their own."""
    seqs = gen.gen(n - dups, L, seed, sub=sub, indel=indel)
    seqs = seqs + seqs[:dups]
    return gen.fasta(seqs)


def run(args):
    return subprocess.run([BIN] + args, check=True, capture_output=True, text=True).stdout


def main():
    os.chdir(HERE)
    out = dict(trees=[], fasta=[])
    for case in TREE_CASES:
        with open("wls.fa.tmp", "w") as f:
            f.write(family(*case))
        rec = dict(zip(("n", "L", "seed", "sub", "indel", "dups"), case))
        rec["W"] = run(["-T", "-i", "0", "-a", "-W", "wls.fa.tmp"])
        rec["WW"] = run(["-T", "-i", "0", "-a", "-WW", "wls.fa.tmp"])
        out["trees"].append(rec)
    for case in FASTA_CASES:
        with open("wls.fa.tmp", "w") as f:
            f.write(family(*case))
        rec = dict(zip(("n", "L", "seed", "sub", "indel", "dups"), case))
        rec["W"] = run(["--fasta", "-a", "-m", "-W", "wls.fa.tmp"])
        out["fasta"].append(rec)
    os.remove("wls.fa.tmp")
    with open("wls.json", "w") as f:
        json.dump(out, f, indent=0)


if __name__ == "__main__":
    main()
