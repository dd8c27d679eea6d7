"""The --topology measurement: `bionj_s` of the plan-driven joins, host loop (PGM_HOST_BIONJ=1) against device
(PGM_DEVICE_BIONJ=1), median of RUNS, on gen.gen(n, 300, 11) for n = 64, 256, 1024 with the family's own tree as the topology and on
the --batch set of DESIGN 4 (512 x 16 x 300) with a topology per family; and the process wall of `pgmsa -a -T -i 0` without
--topology on gen.gen(256, 400, 7), another build of the driver (the parent commit's) against this one.

Usage: measure_topology.py WORKDIR [--parent PGMSA] [--runs 5] [--families 512]
Every run is a child process under a time limit of its own; the first failure ends the script."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen  # noqa: E402
import prographmsa_amd as pg  # noqa: E402


def run(exe, args, env=None, timeout=300):
    t0 = time.perf_counter()
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("%s %s: exit %d\n%s" % (exe, " ".join(args), r.returncode, r.stderr[-2000:]))
    stats = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{")]
    return r.stdout, (stats[0] if stats else {}), wall


def both_paths(args, runs, outputs=None):
    """median bionj_s, device calls and launches of the two paths; the outputs of the two must be identical."""
    row, seen = {}, []
    for path, env in (("host", {"PGM_HOST_BIONJ": "1"}), ("device", {"PGM_DEVICE_BIONJ": "1"})):
        secs = []
        for _ in range(runs):
            out, st, _ = run(pg.PGMSA_PATH, args, env)
            secs.append(st["bionj_s"])
        seen.append(out if outputs is None else [open(p).read() for p in outputs])
        row[path] = dict(bionj_ms=1e3 * statistics.median(secs), all_ms=[round(1e3 * s, 4) for s in secs], calls=st["bionj_device_calls"], launches=st["bionj_launches"])
    assert seen[0] == seen[1], "host and device outputs differ"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workdir")
    ap.add_argument("--parent")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--families", type=int, default=512)
    a = ap.parse_args()
    w = os.path.abspath(a.workdir)
    os.makedirs(w, exist_ok=True)
    for n in (64, 256, 1024):
        fa, tp = os.path.join(w, "n%d.fa" % n), os.path.join(w, "n%d.nwk" % n)
        open(fa, "w").write(gen.fasta(gen.gen(n, 300, 11)))
        open(tp, "w").write(run(pg.PGMSA_PATH, ["-T", "-i", "0", fa])[0])
        print(json.dumps(dict(case="solo", n=n, **both_paths(["-T", "-i", "0", "--stats", "--topology", tp, fa], a.runs))), flush=True)
    bd = os.path.join(w, "batch")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_batch_set.py"), bd, str(a.families), "16", "300", "4242"])
    fams = open(os.path.join(bd, "families.txt")).read().split()
    with open(os.path.join(bd, "trees.list"), "w") as f:
        f.write("".join("%s\t%s.nwk\n" % (p, p) for p in fams))
    run(pg.PGMSA_PATH, ["--batch", os.path.join(bd, "trees.list"), "-T", "-i", "0"])
    outs = [os.path.join(bd, "out", os.path.basename(p) + ".out") for p in fams]
    with open(os.path.join(bd, "topo.list"), "w") as f:
        f.write("".join("%s\t%s\t\t%s.nwk\n" % (p, o, p) for p, o in zip(fams, outs)))
    print(json.dumps(dict(case="batch", families=len(fams), **both_paths(["--batch", os.path.join(bd, "topo.list"), "--fasta", "--stats"], a.runs, outs))), flush=True)
    fa = os.path.join(w, "wall.fa")
    open(fa, "w").write(gen.fasta(gen.gen(256, 400, 7)))
    walls = {}
    for series in range(2):   # the builds alternate: two series of each
        for name, exe in (("parent", a.parent), ("this", pg.PGMSA_PATH)):
            if exe:
                walls.setdefault(name, []).append(round(statistics.median(run(exe, ["-a", "-T", "-i", "0", fa])[2] for _ in range(a.runs)), 4))
    print(json.dumps(dict(case="process_wall_s", **walls)), flush=True)


if __name__ == "__main__":
    main()
