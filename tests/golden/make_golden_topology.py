"""Goldens of --topology (branch lengths on a fixed guide-tree topology; reference src/TreeNJ.cpp:31-130, :158-179).

Usage: python make_golden_topology.py [path/to/ProGraphMSA_64]  ->  topology.json

Tree cases: the twelve NW_TREE_CASES families of make_golden.py, each with NW distances (-a -T -i 0) and with the default k-mer
distances (-T -i 0), and per family six topologies: its own BioNJ tree, that tree with the children swapped at a seeded random
subset of its nodes, a ladder in name order, a ladder in shuffled order, a seeded random binary tree, and a random binary tree
with two extra leaves that are no sequences.  The order in which the reference visits the nodes of the topology shows in the
branch lengths (the swapped and shuffled cases are there to pin it).  Alignment cases: the full default flow (-i 2: the topology
holds for every re-estimation) on c1.fa and x1.fa, and one -t ... -i 1 run.  No -m / -M: their last bits are Eigen's solver's."""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen  # noqa: E402
import topology_ref as T  # noqa: E402

BIN = sys.argv[1] if len(sys.argv) > 1 else "ProGraphMSA_64"

NW_TREE_CASES = [  # (taxa, length, seed, substitution rate, indel rate): those of make_golden.py
    (5, 250, 585126, 0.05, 0.005), (6, 250, 81768, 0.05, 0.005), (7, 120, 59769, 0.1, 0.005), (9, 60, 815905, 0.2, 0.005),
    (9, 250, 4816, 0.1, 0.02), (11, 120, 348741, 0.05, 0.02), (13, 120, 133400, 0.2, 0.02), (16, 120, 653397, 0.2, 0.005),
    (16, 60, 944662, 0.2, 0.005), (16, 250, 545337, 0.1, 0.02), (21, 120, 295589, 0.05, 0.02), (30, 60, 7, 0.1, 0.02)]
FLOWS = dict(nw=["-a", "-T", "-i", "0"], angle=["-T", "-i", "0"])


def run(args):
    return subprocess.run([BIN] + args, check=True, capture_output=True, text=True).stdout


def topologies(names, own, seed):
    """[(kind, topology)] of one family; `own` is the newick of its BioNJ tree."""
    rng = random.Random(seed)
    own = T.parse_newick(own)
    shuffled = list(names)
    rng.shuffle(shuffled)
    return [("own", own), ("swapped", T.swap_children(own, rng)), ("ladder", T.ladder(list(names))), ("ladder_shuffled", T.ladder(shuffled)),
            ("random", T.random_tree(names, rng)), ("extra_leaves", T.random_tree(list(names) + ["extra0", "extra1"], rng))]


def fasta_names(path):
    return [l[1:].strip() for l in open(path) if l.startswith(">")]


def main():
    os.chdir(HERE)
    out = dict(trees=[], fasta=[])
    for (n, L, seed, sub, indel) in NW_TREE_CASES:
        seqs = gen.gen(n, L, seed, sub=sub, indel=indel)
        with open("topo.fa.tmp", "w") as f:
            f.write(gen.fasta(seqs))
        names = ["seq%04d" % i for i in range(n)]
        own = run(["-a", "-T", "-i", "0", "topo.fa.tmp"])
        for kind, topo in topologies(names, own, seed):
            with open("topo.nwk.tmp", "w") as f:
                f.write(T.format_topology(topo) + "\n")
            for flow, flags in FLOWS.items():
                out["trees"].append(dict(n=n, L=L, seed=seed, sub=sub, indel=indel, kind=kind, flow=flow, flags=flags,
                                         topology=T.format_topology(topo), stdout=run(flags + ["--topology", "topo.nwk.tmp", "topo.fa.tmp"])))
    for fa, flags, tree in [("c1.fa", ["--fasta"], None), ("x1.fa", ["--fasta"], None), ("c1.fa", ["--fasta", "-i", "1"], "c1.tree")]:
        names = fasta_names(fa)
        topo = T.random_tree(sorted(names), random.Random(len(names)))
        with open("topo.nwk.tmp", "w") as f:
            f.write(T.format_topology(topo) + "\n")
        args = flags + (["-t", tree] if tree else []) + ["--topology", "topo.nwk.tmp", fa]
        out["fasta"].append(dict(fasta=fa, flags=flags, tree=tree, topology=T.format_topology(topo), stdout=run(args)))
    os.remove("topo.fa.tmp")
    os.remove("topo.nwk.tmp")
    with open("topology.json", "w") as f:
        json.dump(out, f, indent=0)


if __name__ == "__main__":
    main()
