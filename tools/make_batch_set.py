"""Seeded set of small families for the `pgmsa --batch` measurement: N families of n sequences x L residues.

Usage: make_batch_set.py DIR [N=512] [n=16] [L=300] [SEED=4242]
Writes DIR/fam%04d.fa, DIR/families.list (input<TAB>output under DIR/out/) and DIR/families.txt (the FASTA paths, one per line)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gen  # noqa: E402


def main():
    d = sys.argv[1]
    N, n, L, seed = [int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((2, 512), (3, 16), (4, 300), (5, 4242))]
    os.makedirs(os.path.join(d, "out"), exist_ok=True)
    fams = []
    for k in range(N):
        p = os.path.join(d, "fam%04d.fa" % k)
        with open(p, "w") as f:
            f.write(gen.fasta(gen.gen(n, L, seed + k)))
        fams.append(p)
    with open(os.path.join(d, "families.list"), "w") as f:
        for k, p in enumerate(fams):
            f.write("%s\t%s\n" % (p, os.path.join(d, "out", "fam%04d.out" % k)))
    with open(os.path.join(d, "families.txt"), "w") as f:
        f.write("\n".join(fams) + "\n")


if __name__ == "__main__":
    main()
