#!/usr/bin/env python3
"""bench.py — DP cell-updates/s of the alignGraphs hot path on the BASELINE workload (256 seqs x 1000 aa, WAG).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

`python bench.py --gpus N` without a launcher (WORLD_SIZE unset, N > 1) starts that launcher itself, before anything
touches a GPU, and passes its output through.

Workload (config.workload): the 255 graph-vs-graph alignGraphs jobs of one progressive pass over the synthetic
256 x 1000 aa family (tests/gen.py seed 3, guide tree tests/golden/c3.tree, --mldist), 2.71e8 DP cells, exactly the
jobs the product driver issues (captured with `pgmsa --dump_jobs` on this GPU during untimed set-up).
One "step" = one pass of the hot path over that batch with the inputs resident in HBM: prep (float casts,
T = M^T g2) + emission scores + the fill kernel (DP fill of every band and, after a job's last band, its traceback),
then the result/mapping copy back to the host.

A plain run does what the headline figure needs and no more: it captures the jobs (one run of the driver), builds the batch,
warms up, times the steps, writes --dump-outputs and prints the result line (value, ms_per_step and `roofline`, the stage times
that the library's HIP events recorded during those same steps).  Every other record takes runs of its own and is measured
with --full only: the driver's own times (end_to_end, default_flow, roofline_pass), the leaf level (roofline_leaf), the
all-pairs and context-profile satellites, configs 4 / 5, the strong-scaling legs and the CPU baseline.

Multi-GPU: one process per GPU, no collective on the data path and no RCCL anywhere (torch.distributed with the gloo backend
only provides the barrier, the max-over-ranks clock and the rendezvous store that serves the work queue's ticket counter).
  value              every rank runs the headline batch on its own device (weak scaling of independent batches)
  all_pairs_nw*      STRONG scaling of the all-pairs stage (DistanceFactoryAlign): the alignPair jobs of the family, cut into
                     tiles (longest first) that the ranks pull from one atomic ticket counter (prographmsa_amd/farm.py, the
                     process-per-GPU twin of the product's farm in host/distance.cpp); 256 x 1000 and 1024 x 600 families
  progressive_strong STRONG scaling of the progressive pass: (a) the product driver itself on all N GPUs (rank 0 runs `pgmsa` with
                     PGM_DEVICES = every rank's device: the jobs of a guide-tree level, the leaves and the merges are dealt to one
                     context per GPU, host/graph_align.cpp farm_shards), (b) the 255 captured jobs dealt to the ranks (longest
                     first); both bounded by the root job's critical path, reported as measured
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (a step is ~4.7 ms; this pool's hosts stall a GPU wait for ~20 ms about once a second, whatever runs — tools/probe_step.py —
    # so a 20-step region either misses the stall or carries 1 ms of it per step; 200 steps carry their share)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nseq", type=int, default=256, help="debug: smaller family (changes the workload; not the headline)")
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure every other record (driver times, leaf level, satellites, configs 4 / 5, strong scaling, CPU baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the sub-records (configs 4 / 5, 1024 x 600 all-pairs, strong scaling)")
    ap.add_argument("--only-headline", action="store_true", help="the timed loop over the headline batch and nothing else (profiling runs: every kernel launch of the process belongs to a step)")
    ap.add_argument("--only-satellites", action="store_true", help="profiling runs: the all-pairs alignPair stage and the context-profile call of the headline family, nothing else timed")
    ap.add_argument("--only-config", default=None, choices=["c4", "c5"], help="profiling runs: three passes over the jobs of BASELINE config 4 / 5 and nothing else")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU, no compute: only the launch / rendezvous / work-queue / aggregation plumbing (gloo), for CPU rehearsals")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the results of the last one as DIR/<name>.npy (rank 0), to compare two builds output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.dry_run or args.only_config):
        ap.error("--dump-outputs needs the timed loop over the headline batch (not with --dry-run or --only-config)")
    return args


DUMP_CAP_BYTES = 60 << 20   # array bytes of --dump-outputs: with the .npy headers under 64 MB in all


def dump_outputs(out_dir, results):
    """What a caller of the timed path receives from its last step (pgm_align_batch_fetch: per job the score, status, n_tr_indels
    and the two node mappings) as float32 / float64 .npy files.  The mappings of the jobs are concatenated in job order (map_len:
    each job's share); their uint32 values, PGM_GAP included, are exact in float64.  Above DUMP_CAP_BYTES in all, a fixed seeded
    sample of the jobs is written (job: their indices in the batch)."""
    import numpy as np
    lens = np.array([len(r["map1"]) for r in results], np.int64)
    job = np.arange(len(results))
    if 16 * lens.sum() + 40 * len(results) > DUMP_CAP_BYTES:
        order = np.random.default_rng(0).permutation(len(results))
        job = np.sort(order[np.cumsum(16 * lens[order] + 40) <= DUMP_CAP_BYTES])
    sel = [results[i] for i in job]
    arrays = {"job": job.astype(np.float64),
              "score": np.array([r["score"] for r in sel], np.float32),
              "status": np.array([r["status"] for r in sel], np.float64),
              "n_tr_indels": np.array([r["n_tr_indels"] for r in sel], np.float64),
              "map_len": lens[job].astype(np.float64),
              "map1": np.concatenate([r["map1"] for r in sel]).astype(np.float64),
              "map2": np.concatenate([r["map2"] for r in sel]).astype(np.float64)}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def launch_ranks(args):
    """`bench.py --gpus N` without a launcher: start one process per GPU through torch.distributed.run (before any GPU call)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    args = parse_args()
    if args.only_satellites:
        args.steps, args.warmup, args.no_extra, args.no_cpu_baseline = 1, 1, True, True
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")

    import torch
    import torch.distributed as dist
    from prographmsa_amd import farm

    if args.dry_run:
        # plumbing rehearsal: rendezvous, ticket queue, barrier, max-over-ranks clock, sum of the units; nothing is computed
        if world > 1:
            dist.init_process_group("gloo")
        q = farm.TicketQueue("dry_tiles", world)
        ntiles, mine = 64, []
        while True:
            t = q.next()
            if t >= ntiles:
                break
            mine.append(t)
            time.sleep(0.001)
        units = torch.tensor([float(len(mine))], dtype=torch.float64)
        clock = torch.tensor([1.0 + rank], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(units, op=dist.ReduceOp.SUM)
            dist.all_reduce(clock, op=dist.ReduceOp.MAX)
            gathered = [None] * world
            dist.all_gather_object(gathered, mine)
        else:
            gathered = [mine]
        if rank == 0:
            once = sorted(t for g in gathered for t in g) == list(range(ntiles))
            print(json.dumps({"metric": "DP cell-updates/sec (GCUPS) + wall-clock on 256 seqs × 1000 aa, WAG", "value": None, "unit": "GCUPS",
                              "n_gpus": world, "steps": 0, "warmup": 0, "dry_run": True, "tiles": ntiles, "tiles_pulled": int(units.item()),
                              "every_tile_exactly_once": once, "max_clock": clock.item()}))
        if world > 1:
            dist.destroy_process_group()
        return

    torch.cuda.set_device(local_rank)
    if world > 1:
        dist.init_process_group("gloo")   # barrier, clock reduction and the work queue's store: control path only, no RCCL

    import ctypes as C
    import hashlib
    import numpy as np
    import gen
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J

    ctx = pg.Context(local_rank)
    devname, cus = ctx.device_info()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    md5s = json.load(open(os.path.join(ROOT, "tests", "golden", "md5.json")))

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world > 1:
            t = torch.tensor([x], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return x

    def sum_over_ranks(x):
        if world > 1:
            t = torch.tensor([x], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return float(t.item())
        return x

    # ---- untimed set-up: produce the jobs with the product driver on this GPU --------------------
    tmp = tempfile.mkdtemp(prefix="pgm_bench_r%d_" % rank)
    env = dict(os.environ, PGM_DEVICE=str(local_rank))

    def capture(fasta_text, flags, name):
        """Runs pgmsa on a family (untimed), returns (jobs, stats, md5 of the FASTA it printed)."""
        fa = os.path.join(tmp, name + ".fa")
        with open(fa, "w") as f:
            f.write(fasta_text)
        dump = os.path.join(tmp, name + ".jobs")
        r = subprocess.run([pg.PGMSA_PATH] + flags + ["--dump_jobs", dump, "--stats", fa], capture_output=True, text=True, env=env)
        if r.returncode != 0:
            raise SystemExit("pgmsa failed: " + r.stderr)
        js = J.load_jobs(dump)
        os.remove(dump)
        # the driver's own times come from further runs without the job dump (writing the jobs to disk is not part of the
        # product): the median of three by progressive_s, all three listed (a pass is 50-150 ms, and this pool's hosts stall a GPU
        # wait for ~20 ms about once a second — on some boxes several times per pass: DESIGN §4)
        runs = []
        if rank != 0 or not args.full:   # (only rank 0 of a --full run reports the driver's times)
            st = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith('{"backend"')][-1])
            st["wall_s"] = None
            return js, st, hashlib.md5(r.stdout.encode()).hexdigest()
        for _ in range(3):
            t0 = time.time()
            r2 = subprocess.run([pg.PGMSA_PATH] + flags + ["--stats", fa], capture_output=True, text=True, env=env)
            wall = time.time() - t0
            if r2.returncode != 0 or r2.stdout != r.stdout:
                raise SystemExit("pgmsa: repeated run failed or differs: " + r2.stderr)
            st = json.loads([ln for ln in r2.stderr.splitlines() if ln.startswith('{"backend"')][-1])
            st["wall_s"] = round(wall, 3)
            runs.append(st)
        st = sorted(runs, key=lambda q: q["progressive_s"])[1]   # the median of the three runs
        st["progressive_s_of_3_runs"] = sorted(q["progressive_s"] for q in runs)
        return js, st, hashlib.md5(r.stdout.encode()).hexdigest()

    headline = (args.nseq == 256 and args.len == 1000)
    fam = gen.gen(args.nseq, args.len, 3)
    if headline:
        tree_args = ["-t", os.path.join(ROOT, "tests", "golden", "c3.tree")]
    else:   # debug sizes: NW guide tree from the GPU all-pairs stage
        fa0 = os.path.join(tmp, "t.fa")
        open(fa0, "w").write(gen.fasta(fam))
        tr = subprocess.run([pg.PGMSA_PATH, "-a", "-m", "-T", "-i", "0", fa0], capture_output=True, text=True, env=env, check=True).stdout
        with open(os.path.join(tmp, "t.tree"), "w") as f:
            f.write(tr)
        tree_args = ["-t", os.path.join(tmp, "t.tree")]
    if args.only_config:   # profiling runs (tools/profile_bench.sh): the jobs of one pass of BASELINE config 4 / 5, three launches
        gold = os.path.join(ROOT, "tests", "golden")
        text, flags = {"c4": (gen.fasta(gen.gen_codon(128, 1000, 4)), ["--codon", "--fasta", "-t", os.path.join(gold, "c4.tree")]),
                       "c5": (gen.fasta(gen.gen(1024, 600, 6)), ["--fasta", "-t", os.path.join(gold, "c5.tree")])}[args.only_config]
        js, st, md5 = capture(text, flags, args.only_config)
        b2 = J.Batch(ctx, js)
        for _ in range(3):
            b2.run(); b2.fetch_raw()
        print(json.dumps({"only_config": args.only_config, "jobs": len(js), "cells": b2.cells, "launches": 3, "ms": [round(v, 3) for v in b2.stage_times(reset=True)[:3]]}))
        b2.close(); ctx.close()
        return
    jobs, stats, out_md5 = capture(gen.fasta(fam), ["--fasta", "-m"] + tree_args, "c3")
    # the reference's default flow from sequences alone (`--fasta -a`: all-pairs guide tree, two rounds of progressive
    # alignment + guide-tree re-estimation, final alignment), rank 0 only; the FASTA's md5 is checked against the fixture of
    # the reference binary's output for the headline family
    default_flow = None
    if rank == 0 and args.full:
        fa0 = os.path.join(tmp, "c3.fa")
        t0 = time.time()
        r2 = subprocess.run([pg.PGMSA_PATH, "--fasta", "-a", "--stats", fa0], capture_output=True, text=True, env=env)
        dt2 = time.time() - t0
        if r2.returncode == 0:
            st2 = json.loads([ln for ln in r2.stderr.splitlines() if ln.startswith('{"backend"')][-1])
            default_flow = {"cmd": "pgmsa --fasta -a", "wall_s": round(dt2, 3), "init_s": st2.get("init_s"), "tree_s": st2["tree_s"], "progressive_s": st2["progressive_s"],
                            "align_cells": st2["align_cells"], "nw_cells": st2["nw_cells"]}
            if headline:
                default_flow["fasta_identical_to_reference"] = (hashlib.md5(r2.stdout.encode()).hexdigest() == md5s.get("c3.a_iter.out.fa"))
                default_flow["reference_wall_s"] = 919   # bin/ProGraphMSA_64 --fasta -a, one core of the build container
    batch = J.Batch(ctx, jobs)
    cells = batch.cells

    for _ in range(args.warmup):
        batch.run()
        batch.fetch_raw()
    if args.warmup > 0:
        check = batch.fetch()   # results of the last warm-up step as Python objects (sanity check)
        assert all(r["status"] == 0 and len(r["map1"]) > 0 for r in check)
    batch.stage_times(reset=True)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        batch.run()          # pgm_align_batch_run: prep + emission + fill (+ lean) / traceback kernels
        batch.fetch_raw()    # pgm_align_batch_fetch: wait, D2H of scores and mappings into the caller's buffers
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    total_cells = sum_over_ranks(float(cells) * args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, batch.cj.results())   # the caller buffers still hold the last timed step's results

    # ---- roofline of the dominant kernel (pgm_fill_kernel beside pgm_lean_kernel: DP fill + tracebacks): HIP events on the
    # library's stream, recorded by every launch of the timed loop above and averaged over exactly those launches ----
    ms_prep, ms_emis, ms_fill, n_timed = batch.stage_times(reset=True)
    assert n_timed == args.steps
    alg_bytes = 16.0 * cells            # one float4 {M,X,W,Y} store per cell; S is materialised by the emission
    achieved = alg_bytes / (ms_fill * 1e-3) / 1e9   # kernel, so this kernel also reads 4 B/cell that are not counted here
    # HBM traffic per launch from the PMC passes of tools/profile_bench.sh (FETCH_SIZE, WRITE_SIZE in KB; gfx950: reads doubled)
    traffic, traffic_step, pmc_name = None, None, "profiles/r4_pmc.json"
    pmc_path = os.path.join(ROOT, pmc_name)
    FILL_STAGE = ("pgm_fill_kernel", "pgm_crit_kernel", "pgm_band_kernel", "pgm_lean_kernel", "pgm_tb_kernel")   # the kernels between the events of the fill stage
    STEP = FILL_STAGE + ("pgm_prep_kernel", "pgm_emission_skew_kernel")

    def pmc_bytes(allp, names):
        """HBM bytes per step of the kernels `names` in a profiled run: 2 x FETCH_SIZE (gfx950 counts half of a streaming read) + WRITE_SIZE."""
        steps_prof = float(allp.get("_steps", 0))
        kb = 0.0
        for k, v in allp.items():
            if isinstance(v, dict) and k.startswith(names) and "FETCH_SIZE" in v and "WRITE_SIZE" in v:
                kb += 2.0 * v["FETCH_SIZE"]["total_kb"] + v["WRITE_SIZE"]["total_kb"]
        return round(kb * 1024.0 / steps_prof) if kb and steps_prof else None
    if headline and os.path.exists(pmc_path):
        allp = json.load(open(pmc_path))
        traffic = pmc_bytes(allp, FILL_STAGE)       # all launches of the stage's kernels in the profiled run (bench.py --only-headline), per step
        traffic_step = pmc_bytes(allp, STEP)        # ... with the prep and emission kernels in front of the stage
    pmc_all = json.load(open(pmc_path)) if os.path.exists(pmc_path) else {}
    pmc_sat_path = os.path.join(ROOT, "profiles/r4_satellites_pmc.json")   # the same passes over `bench.py --only-satellites`
    if os.path.exists(pmc_sat_path):
        for k, v in json.load(open(pmc_sat_path)).items():
            if isinstance(v, dict) and k.startswith(("pgm_nw_kernel", "pgm_csprofile_kernel")):
                pmc_all[k] = v

    def valu_roofline(kernel, launch_ms):
        """VALU issue rate of a compute-bound satellite kernel: SQ_INSTS_VALU of one launch (profiles/r2_pmc.json, rocprofv3
        --pmc pass of tools/profile_bench.sh) over the launch time measured live, against the chip's issue peak of one
        wave64 VALU instruction per 2 cycles and SIMD (1024 SIMDs, 2.4 GHz nominal)."""
        c = next((v for k, v in pmc_all.items() if k.startswith(kernel)), None)
        if not c or "SQ_INSTS_VALU" not in c or launch_ms <= 0:
            return None
        insts = c["SQ_INSTS_VALU"]["mean"]
        peak = 1024 * 2.4e9 / 2.0
        return {"bound": "valu_issue", "achieved": round(insts / (launch_ms * 1e-3) / 1e9, 1), "peak": round(peak / 1e9, 1), "unit": "G wave-instr/s",
                "frac": round(insts / (launch_ms * 1e-3) / peak, 4), "valu_insts_per_launch": insts,
                "lds_bank_conflict_cycles_per_lds_inst": round(c["SQ_LDS_BANK_CONFLICT"]["mean"] / max(c["SQ_INSTS_LDS"]["mean"], 1.0), 2),
                "wave_cycles_split": {k: round(c[k]["mean"] / c["SQ_WAVE_CYCLES"]["mean"], 3) for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY") if k in c},
                "source": pmc_name + " (SQ pass), launch time live (HIP events)"}

    # who the stage waits for: the last launch's per-job timeline (pgm_align_batch_job_times), relative to the start of the stage
    tl = None
    try:
        import ctypes as C_
        tk = np.zeros(2 * len(jobs), np.uint64)
        pg.check(pg.lib.pgm_align_batch_job_times(ctx.handle, batch.handle, tk.ctypes.data_as(C_.POINTER(C_.c_uint64))))
        tk = tk.reshape(-1, 2).astype(np.float64) / 100.0
        off = ms_fill * 1e3 - tk.max()
        n1s = np.array([j.g1.n for j in jobs])
        chain = np.array([j.g1.e_col.size == j.g1.n - 1 and j.g2.e_col.size == j.g2.n - 1 for j in jobs])
        big = int(np.argmax(n1s * np.array([j.g2.n for j in jobs])))
        tl = {"note": "end of the last timed launch's sweeps / tracebacks per kind of job, us after the start of the stage (mean stage time as origin)",
              "leaf_jobs_done": round(float((tk[chain, 1] + off).max())) if chain.any() else None,
              "jobs_below_1216_rows": {"sweeps": round(float((tk[~chain & (n1s < 1217), 0] + off).max())), "tracebacks": round(float((tk[~chain & (n1s < 1217), 1] + off).max()))} if (~chain & (n1s < 1217)).any() else None,
              "largest_job": {"rows_x_cols": "%d x %d" % (jobs[big].g1.n, jobs[big].g2.n), "sweeps": round(float(tk[big, 0] + off)), "traceback": round(float(tk[big, 1] + off))}}
    except Exception as e:   # (an older library without the entry point)
        tl = {"error": str(e)}
    roofline = {"bound": "hbm", "kernel": "fill stage: pgm_crit_kernel (two launches: the longest chains on sixteen wavefronts per band, the other jobs of 20 and more bands), "
                                          "pgm_band_kernel (narrow and wide bands) and pgm_lean_kernel side by side, an instance of pgm_tb_kernel (tracebacks) behind each of the first three",
                "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s",
                "frac": round(achieved / 8000.0, 5), "traffic": traffic, "traffic_whole_step": traffic_step, "algorithmic_bytes": alg_bytes, "timeline_us": tl,
                "traffic_source": pmc_name + " (rocprofv3 --pmc, separate passes over `bench.py --only-headline`; bytes per step = sum over the stage's kernel launches of 2 x FETCH_SIZE + WRITE_SIZE; "
                                             "traffic_whole_step: the same with pgm_prep_kernel and pgm_emission_skew_kernel, which write and re-read the emission scores)",
                "ms": {"prep": round(ms_prep, 4), "emission": round(ms_emis, 4), "fill_and_traceback": round(ms_fill, 4),
                       "sum": round(ms_prep + ms_emis + ms_fill, 4), "source": "HIP events of the %d timed steps themselves (pgm_align_batch_stage_times)" % n_timed},
                "fill_gcups": round(cells / (ms_fill * 1e-3) / 1e9, 3)}

    if args.only_headline:
        if rank == 0:
            print(json.dumps({"metric": "DP cell-updates/sec (GCUPS), headline batch only", "value": round(total_cells / dt / 1e9, 4), "unit": "GCUPS", "n_gpus": world, "steps": args.steps,
                              "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "roofline": roofline}))
        return
    head = {
        "metric": "DP cell-updates/sec (GCUPS) + wall-clock on 256 seqs × 1000 aa, WAG",
        "value": round(total_cells / dt / 1e9, 4), "unit": "GCUPS",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%d seqs x %d aa, WAG, --mldist: the %d alignGraphs jobs of one progressive pass "
                               "(%.3e DP cells) per GPU, inputs resident in HBM" % (args.nseq, args.len, len(jobs), cells),
                   "headline": headline, "device": devname, "cus": cus, "jobs": len(jobs), "cells_per_step": cells},
        "roofline": roofline,
    }
    if not (args.full or args.only_satellites):   # a plain run ends here: every record below takes runs of its own
        if rank == 0:
            print(json.dumps(head))
        batch.close()
        ctx.close()
        if world > 1:
            dist.destroy_process_group()
        return
    # ---- the two other lines SURVEY section 7 asks for: the leaf level alone, and the product's whole progressive pass --------
    def is_chain(g):
        return g.r_col is None and g.e_col.size == g.n - 1 and bool(np.all(g.e_col == np.arange(g.n - 1, dtype=np.uint32))) and bool(np.all(g.e_val != 0))
    leaf_jobs = [] if args.only_satellites else [j for j in jobs if is_chain(j.g1) and is_chain(j.g2)]
    roofline_leaf = None
    if leaf_jobs:
        lb = J.Batch(ctx, leaf_jobs)
        for _ in range(3):
            lb.run(); lb.fetch_raw()
        lb.stage_times(reset=True)
        tl = time.perf_counter()
        nrep = max(20, args.steps // 4)
        for _ in range(nrep):
            lb.run(); lb.fetch_raw()
        ldt = (time.perf_counter() - tl) / nrep
        lp, le, lf, _n = lb.stage_times(reset=True)
        lcells = lb.cells
        roofline_leaf = {"bound": "hbm", "kernel": "pgm_lean_kernel", "jobs": len(leaf_jobs), "cells": lcells, "ms_per_step": round(ldt * 1e3, 4),
                         "ms": {"prep": round(lp, 4), "emission": round(le, 4), "fill_and_traceback": round(lf, 4)},
                         "gcups": round(lcells / (lf * 1e-3) / 1e9, 2), "achieved": round(16.0 * lcells / (lf * 1e-3) / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                         "frac": round(16.0 * lcells / (lf * 1e-3) / 8e12, 5),
                         "binding": {"valu_issue": valu_roofline("pgm_lean_kernel", lf),
                                     "hbm_bytes_per_launch_in_the_headline_batch": (pmc_bytes({k: v for k, v in pmc_all.items()}, ("pgm_lean_kernel",)) if pmc_all.get("_steps") else None),
                                     "note": "the bound that binds this kernel is vector issue and the LDS hand-off between its wavefronts, not HBM: its VALU issue fraction, and the HBM bytes one "
                                             "launch moves in the headline batch (profiles/r4_pmc.json) for comparison with the 16 B per cell of the notional figure"},
                         "note": "the chain-only jobs of the pass (sequence graph against sequence graph: the guide tree's leaf level) as a batch of their own; "
                                 "algorithmic bytes as for the headline (16 B per cell); these jobs keep 4 decision bits per cell instead of the four floats "
                                 "(DESIGN section 3.1), so the bytes actually moved are far fewer: S read 4 B + 0.5 B per cell"}
        lb.close()
    roofline_pass = {"bound": "hbm", "what": "the product driver's whole progressive pass (pgmsa --fasta -m -t: 8 level-batched calls, host merges, H2D / D2H)",
                     "progressive_s": stats["progressive_s"], "gcups": round(cells / stats["progressive_s"] / 1e9, 3),
                     "achieved": round(16.0 * cells / stats["progressive_s"] / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                     "frac": round(16.0 * cells / stats["progressive_s"] / 8e12, 5)}

    # ---- strong scaling of the progressive pass: the same jobs dealt to the ranks (longest first), one pass ---------------
    prog_strong = None
    if world > 1 and not args.no_extra:
        shards = farm.lpt_shards([j.cells for j in jobs], world)
        mine = [jobs[i] for i in shards[rank]]
        sb = J.Batch(ctx, mine)
        sb.run(); sb.fetch_raw()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sb.run()
            sb.fetch_raw()
        barrier()
        sdt = max_over_ranks(time.perf_counter() - t0)
        product = None
        barrier()
        if rank == 0:   # the product driver's own farm: one context per GPU inside ONE process (the other ranks wait at the barrier)
            envp = dict(os.environ, PGM_DEVICES=",".join(str(d) for d in range(world)))
            envp.pop("PGM_DEVICE", None)
            fa0 = os.path.join(tmp, "c3.fa")
            runs = []
            for _ in range(3):
                rp = subprocess.run([pg.PGMSA_PATH, "--fasta", "-m"] + tree_args + ["--stats", fa0], capture_output=True, text=True, env=envp)
                if rp.returncode == 0:
                    stp = json.loads([ln for ln in rp.stderr.splitlines() if ln.startswith('{"backend"')][-1])
                    runs.append((stp["progressive_s"], stp.get("farm_level_workers"), hashlib.md5(rp.stdout.encode()).hexdigest() == out_md5))
            if runs:
                runs.sort()
                product = {"cmd": "pgmsa --fasta -m -t (PGM_DEVICES = all %d GPUs)" % world, "progressive_s_of_3_runs": [r[0] for r in runs], "progressive_s": runs[1 if len(runs) > 2 else 0][0],
                           "farm_level_workers": runs[0][1], "fasta_identical_to_one_gpu": all(r[2] for r in runs), "one_gpu_progressive_s": stats["progressive_s"]}
        barrier()
        prog_strong = {"product_farm": product, "jobs_per_rank": [len(s) for s in shards], "ms_per_pass": round(sdt / args.steps * 1e3, 4),
                       "gcups": round(cells * args.steps / sdt / 1e9, 3), "scaling": "strong",
                       "note": "one pass = all 255 jobs across the ranks; the root job (1.7 % of the cells) is a single critical path"}
        sb.close()

    # ---- all-pairs stage (DistanceFactoryAlign, `-a`): alignPair tiles pulled by the ranks from one ticket counter --------
    score = np.loadtxt(os.path.join(ROOT, "prographmsa_amd", "host", "data", "nw_aa.imat"), skiprows=1, dtype=np.int32).reshape(-1)
    order = "ACDEFGHIKLMNPQRSTVWY"

    def all_pairs_stage(seqs_aa, tag):
        enc = [np.array([order.index(c) for c in (s[1:] if s.startswith("M") else s)], np.int8) for s in seqs_aa]
        lens = [len(e) for e in enc]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        syms = np.concatenate(enc).astype(np.int8)
        pairs = farm.sorted_pairs(lens)
        npairs = len(pairs)
        pi_all = np.array([p[0] for p in pairs], np.uint32)
        pj_all = np.array([p[1] for p in pairs], np.uint32)
        tile = farm.tile_size(npairs, world, os.environ.get("PGM_NW_TILE"))
        ntiles = (npairs + tile - 1) // tile
        # result buffers of the rank's tiles in pinned memory (pgm_host_alloc: the D2H copies write them directly), two tiles in flight
        cbuf = [pg.lib.pgm_host_alloc(tile * 400 * 4) for _ in range(2)]
        gbuf = [pg.lib.pgm_host_alloc(tile * 4) for _ in range(2)]
        kernel_ms = [0.0]

        def submit(t, k):
            p0, cnt = t * tile, min(tile, npairs - t * tile)
            ticket = C.c_int(-1)
            pg.check(pg.lib.pgm_nw_pairs_submit(ctx.handle, 20, P(score, C.c_int32), -10, -2, len(enc), P(syms, C.c_int8), P(offs, C.c_uint32),
                                                cnt, P(pi_all[p0:], C.c_uint32), P(pj_all[p0:], C.c_uint32), 0, C.cast(cbuf[k], C.POINTER(C.c_int32)),
                                                C.cast(gbuf[k], C.POINTER(C.c_uint32)), C.byref(ticket)))
            return ticket.value, float(sum(lens[a] * lens[b] for a, b in pairs[p0:p0 + cnt]))

        def run(qname, in_flight):
            # in_flight = 2: the product's loop (host/distance.cpp) — submit tile k+1, then wait for tile k; 1: one tile at a time,
            # which is what the kernel times are taken from (the kernels of overlapping tiles share the device)
            q = farm.TicketQueue(qname, world)
            done_cells, done_tiles, pending = 0.0, 0, None
            kernel_ms[0] = 0.0
            while True:
                t = q.next()
                if t >= ntiles:
                    break
                ticket, cells = submit(t, done_tiles & 1)
                if in_flight == 1:
                    pg.check(pg.lib.pgm_nw_pairs_wait(ctx.handle, ticket))
                    kernel_ms[0] += float(pg.lib.pgm_nw_last_kernel_ms(ctx.handle))
                else:
                    if pending is not None:
                        pg.check(pg.lib.pgm_nw_pairs_wait(ctx.handle, pending))
                    pending = ticket
                done_cells += cells
                done_tiles += 1
            if pending is not None:
                pg.check(pg.lib.pgm_nw_pairs_wait(ctx.handle, pending))
            return done_cells, done_tiles
        run(tag + "_warm", 2)
        barrier()
        t0 = time.perf_counter()
        k_cells, k_tiles = run(tag + "_serial", 1)
        barrier()
        wall_serial = max_over_ranks(time.perf_counter() - t0)
        kms, ktiles = kernel_ms[0], k_tiles
        barrier()
        t0 = time.perf_counter()
        my_cells, my_tiles = run(tag + "_timed", 2)
        barrier()
        wall = max_over_ranks(time.perf_counter() - t0)
        for b_ in cbuf + gbuf:
            pg.lib.pgm_host_free(b_)
        tot = sum_over_ranks(my_cells)
        tiles_per_rank = [my_tiles]
        if world > 1:
            tiles_per_rank = [None] * world
            dist.all_gather_object(tiles_per_rank, my_tiles)
        # rank 0's kernel time for the tiles it took in the serial pass, scaled to the tiles of the timed pass (the ticket queue may
        # deal a rank a different number of tiles in the two passes)
        k_scaled = kms * (my_cells / max(k_cells, 1.0))
        return {"pairs_total": npairs, "cells_total": tot, "tile_pairs": tile, "tiles": ntiles, "tiles_per_rank": tiles_per_rank,
                "wall_s": round(wall, 4), "gcups_wall": round(tot / wall / 1e9, 2), "rank0_kernel_ms": round(k_scaled, 3),
                "rank0_wall_over_kernel": round(wall * 1e3 / max(k_scaled, 1e-9), 3),
                "one_tile_at_a_time": {"wall_s": round(wall_serial, 4), "rank0_kernel_ms": round(kms, 3), "rank0_tiles": ktiles,
                                       "rank0_fixed_ms_per_call": round((wall_serial * 1e3 - kms) / max(ktiles, 1), 3)},
                "rank0_kernel_gcups": round(k_cells / max(kms, 1e-9) / 1e6, 2), "scaling": "strong",
                "note": "tiles of alignPair jobs (longest first) pulled by the ranks from one ticket counter, two tiles in flight per rank "
                        "(pgm_nw_pairs_submit / _wait: D2H of the 400-int count matrices of tile k under the kernel of tile k+1, results "
                        "straight into pinned buffers); wall incl. H2D of the sequences and all D2H; kernel time from a pass with one tile at "
                        "a time; 2 direction bits/cell stored (reference formulation: 12 B/cell)"}
    nw = all_pairs_stage(fam, "nw_c3")
    if headline and world == 1:
        nw["roofline"] = valu_roofline("pgm_nw_kernel", nw["rank0_kernel_ms"] / max(nw["tiles"], 1))
    nw_big = None
    if headline and not args.no_extra:
        nw_big = all_pairs_stage(gen.gen(1024, 600, 6), "nw_c5")
        nw_big["family"] = "1024 x 600 aa (BASELINE config 5 inputs): 523 776 pairs"

    # ---- context-specific leaf profiles (CSProfile::createProfile) at the scale of BASELINE config 5: a synthetic library
    # of K = 4000 context profiles (13 columns), the leaves of a 1024 x 600 aa family sharded over the ranks --------------
    cs = None
    if headline:
        rng = np.random.default_rng(5)
        K, ncols, nleaf, L = 4000, 13, 1024, 600
        p = rng.gamma(0.3, 1.0, (K, ncols, 20)) + 1e-4
        p /= p.sum(2, keepdims=True)
        w = 1.3 * 0.9 ** np.abs(np.arange(ncols) - ncols // 2)
        lp = np.zeros((K, ncols, 21))
        lp[:, :, :20] = np.log(p) * w[None, :, None]
        lpf = np.ascontiguousarray(lp, np.float64).reshape(-1)
        cf = np.ascontiguousarray(p[:, ncols // 2, :], np.float64).reshape(-1)
        prf = np.log(rng.dirichlet(np.ones(K)))
        lo, hi = farm.shard_range(nleaf, rank, world)
        nl = hi - lo
        syms_cs = rng.integers(0, 20, nl * L).astype(np.int8)
        offs_cs = (np.arange(nl + 1) * L).astype(np.uint32)
        out_offs = (np.arange(nl + 1) * 20 * (L + 2)).astype(np.uint64)
        tau = np.full(nl, 0.3)
        pi_cs = np.full(20, 0.05)
        pu_cs = np.full(nl * 20, 0.05)
        out_cs = np.zeros(int(out_offs[-1]))
        pg.check(pg.lib.pgm_csprofile_load(ctx.handle, K, ncols, P(lpf, C.c_double), P(cf, C.c_double), P(prf, C.c_double)))

        def cs_call():
            pg.check(pg.lib.pgm_csprofile_create_batch(ctx.handle, nl, P(syms_cs, C.c_int8), P(offs_cs, C.c_uint32), P(tau, C.c_double),
                                                       P(pi_cs, C.c_double), P(pu_cs, C.c_double), P(out_cs, C.c_double), P(out_offs, C.c_uint64)))
        cs_call()
        barrier()
        t0 = time.perf_counter()
        cs_call()
        barrier()
        cs_dt = max_over_ranks(time.perf_counter() - t0)
        cs_ms = float(pg.lib.pgm_csprofile_last_kernel_ms(ctx.handle))
        flop = 34.0 * K * L * nleaf   # ~K*L*34 flop per sequence (fp64)
        cs_roof = valu_roofline("pgm_csprofile_kernel", cs_ms) if world == 1 else None
        cs = {"roofline": cs_roof, "library": "synthetic K=%d x %d columns" % (K, ncols), "sequences_total": nleaf, "length": L, "wall_s": round(cs_dt, 4),
              "rank0_kernel_ms": round(cs_ms, 3), "gflops_wall": round(flop / cs_dt / 1e9, 1), "scaling": "strong",
              "note": "whole pgm_csprofile_create_batch call incl. H2D of the residues and D2H of the 20 x (L+2) fp64 profiles; "
                      "reference config 5 spends ~450 s of 510 s in createProfile"}

    # ---- BASELINE configs 4 and 5 at full size (rank 0, N = 1): one progressive pass on the committed guide trees ----------
    configs = None
    if headline and rank == 0 and world == 1 and not args.no_extra:
        configs = {}

        def cfg_traffic(name):   # HBM bytes per pass of the fill stage's kernels (profiles/r4_c4_pmc.json / r4_c5_pmc.json: passes over `bench.py --only-config`)
            pth = os.path.join(ROOT, "profiles/r4_%s_pmc.json" % ("c4" if name.startswith("config4") else "c5"))
            return pmc_bytes(json.load(open(pth)), FILL_STAGE) if os.path.exists(pth) else None
        lib_path = os.path.join(tmp, "K4000syn.lib")
        with open(lib_path, "w") as f:
            f.write(gen.genlib(4000, 11))
        gold = os.path.join(ROOT, "tests", "golden")
        for name, text, flags, ref_md5, ref_s in (
                ("config4_128x1000_codons", gen.fasta(gen.gen_codon(128, 1000, 4)), ["--codon", "--fasta", "-t", os.path.join(gold, "c4.tree")], "c4.out.fa", 10),
                ("config5_1024x600_aa", gen.fasta(gen.gen(1024, 600, 6)), ["--fasta", "-t", os.path.join(gold, "c5.tree")], "c5.out.fa", 21),
                ("config5_1024x600_aa_K4000", gen.fasta(gen.gen(1024, 600, 6)),
                 ["--fasta", "-t", os.path.join(gold, "c5.tree"), "--cs_profile", lib_path], "c5.cs.out.fa", 170)):
            js, st, md5 = capture(text, flags, name)
            b2 = J.Batch(ctx, js)
            b2.run(); b2.fetch_raw()
            b2.stage_times(reset=True)
            t0 = time.perf_counter()
            for _ in range(40):
                b2.run()
                b2.fetch_raw()
            d2 = (time.perf_counter() - t0) / 40
            tm = b2.stage_times(reset=True)[:3]
            configs[name] = {"jobs": len(js), "cells": b2.cells, "dim": js[0].g1.dim, "ms_per_pass": round(d2 * 1e3, 3),
                             "gcups": round(b2.cells / d2 / 1e9, 3), "ms": {"prep": round(tm[0], 3), "emission": round(tm[1], 3), "fill_and_traceback": round(tm[2], 3)},
                             "fill_frac_of_hbm_roofline": round(16.0 * b2.cells / (tm[2] * 1e-3) / 8e12, 4),
                             "roofline": {"bound": "hbm", "achieved": round(16.0 * b2.cells / (tm[2] * 1e-3) / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                                          "frac": round(16.0 * b2.cells / (tm[2] * 1e-3) / 8e12, 5), "traffic": cfg_traffic(name)},
                             "pgmsa": {"wall_s": st["wall_s"], "init_s": st.get("init_s"), "progressive_s": st["progressive_s"], "align_call_s": st["align_s"]},
                             "fasta_identical_to_reference": md5 == md5s.get(ref_md5), "reference_one_pass_s": ref_s,
                             "note": "jobs of one progressive pass captured from the product driver, inputs resident in HBM; "
                                     "reference time: bin/ProGraphMSA_64 on one core of the build container"}
            b2.close()

    if args.only_satellites:
        if rank == 0:
            print(json.dumps({"only_satellites": True, "all_pairs_nw": nw, "csprofile": cs}))
        batch.close(); ctx.close()
        return
    out = None
    if rank == 0:
        out = dict(head)
        out.update({
            "roofline_leaf": roofline_leaf,
            "roofline_pass": roofline_pass,
            "all_pairs_nw": nw,
            "all_pairs_nw_1024x600": nw_big,
            "progressive_strong": prog_strong,
            "csprofile": cs,
            "configs": configs,
            "end_to_end": {"pgmsa_wall_s": stats["wall_s"], "init_s": stats.get("init_s"), "progressive_s": stats["progressive_s"], "align_call_s": stats["align_s"],
                           "fasta_identical_to_reference": (out_md5 == md5s.get("c3.out.fa")) if headline else None,
                           "progressive_s_of_3_runs": stats.get("progressive_s_of_3_runs"),
                           "note": "the median of three runs of the product driver outside the timed region (without the job dump; all three under progressive_s_of_3_runs); progressive_s incl. host merges, H2D/D2H and every allocation beyond the context's start-up pool; init_s = HIP start-up + code object load + that pool (128 MB pinned staging, 3.4 GB of device buffers: pgm_ctx_create), before the stage clocks start and inside pgmsa_wall_s",
                           "default_flow": default_flow},
        })
        if world == 1 and not args.no_cpu_baseline:
            import oracle_lib   # test-only CPU restatement, used here solely as the reported CPU baseline
            tc = time.perf_counter()
            passes, ccells = 0, 0
            while passes == 0 or (time.perf_counter() - tc < 10.0 and passes < 8):
                for j in jobs:
                    oracle_lib.align_graphs(j)
                passes += 1
                ccells += sum(j.cells for j in jobs)
            cdt = time.perf_counter() - tc
            cpu_model = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
            out["cpu_baseline"] = {"value": round(ccells / cdt / 1e9, 5), "unit": "GCUPS", "cores": 1, "kind": "port", "host_cpu": cpu_model, "host_cores": os.cpu_count(),
                                   "sample": "%d pass(es) over the same %d-job batch (%.3e cells, %.1f s), oracle/pgm_oracle.c -O2, 1 thread"
                                             % (passes, len(jobs), ccells, cdt)}
        print(json.dumps(out))
    batch.close()
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
