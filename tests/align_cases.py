"""The jobs of the GPU parity tests of alignGraphs (test_gpu_align.py, test_gpu_dims.py) as recipes, importable without a GPU, and
what each of them claims to reach.

Which kernel path a job takes is decided by csrc/pgm_plan.h (plan_job_sweep, finalize_side, plan_schedule) from the graphs' edge
summaries, the other jobs of the batch and the CU count, not by the test.  reach() reads the plan of a batch (the host-only hook
pgm_test_batch_plan through test_cpu_plan.plan) and the graphs' own edge lists and returns the labels below; a case lists the
labels it is there for, test_cpu_align_reach.py holds every case to them at 256 CUs (the MI355X) and every GPU test does the same
at the CU count of its device before it creates the batch.

Labels of a job (a claim such as "narrow+generic" asks for one job with all of them):
  lean | narrow | wide | mode2 | crit3     the sweep: pgm_lean_kernel; a self-contained sweep on a narrow (eight slots) / wide worker
                                           of pgm_band_kernel, by the band list's narrow / wide part; helpers (pgm_fill_kernel);
                                           pgm_crit_kernel
  list:crit | list:rest                    a job of the fill work list: in the launch of the longest chains / in the main launch
  pgm_crit_kernel | pgm_fill_kernel        ... and the kernel that sweeps that launch: pgm_crit_kernel if every job of it is crit3, else
                                           pgm_fill_kernel, which sweeps a crit3 job as the MODE 2 job it also is
  generic kill ov long1 long2 long         nodes of the generic path, interior nodes without predecessors, overflow columns, remote
                                           row entries, long column entries, either of the two
  generic1 generic2                        generic nodes where only graph 1 (rows) / graph 2 (columns) has candidates for them
  nolong                                   mode2 without long1 and long2
  hD16 .. hD64, hDX4 .. hDX32, hDX->8      history depths; crit3 whose X history was raised to 8
  kill1 kill2 kill:row0 kill:row63 kill:endcol   kill nodes of graph 1 / 2, at the first / last row of a band, in the column before END
  inf:chain inf:chain>repeat inf:chain>regular inf:nochain inf:near inf:far inf:long inf:repeat
                                           edges of infinite cost: from node - 1 in front of the finite edge that takes the chain slot
                                           (a repeat edge / a second regular entry) / with none behind it, at distance 2-3, 4-PGM_DCAP, beyond, repeat edges
  dup:d1 dup:d2 dup:d3 dup:far             a repeat edge from the node of a regular edge at that distance
Labels of a batch ("batch:" in a claim): ncrit, narrow bands, wide bands, wide workers, promote 0x8 | promote 0xffffffff, crit_c3, rest_c3."""
import os
import re

import numpy as np

import test_cpu_plan as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256   # the MI355X


def device_limits():
    """the limits of csrc/pgm_device.h the recipes are placed against (a changed limit moves a recipe: the reach test then fails)"""
    text = open(os.path.join(ROOT, "prographmsa_amd", "csrc", "pgm_device.h")).read()
    out = {}
    for name in ("PGM_KF", "PGM_KF8", "PGM_DCAP", "PGM_VL", "PGM_REMOTE_MAX", "PGM_NLONG", "PGM_OV_ENT", "PGM_OV_REC", "PGM_ROWS"):
        out[name] = int(re.search(r"^#define %s\s+(\d+)" % name, text, re.M).group(1))
    return out


LIM = device_limits()
DCAP = LIM["PGM_DCAP"]
ROW_ENTRIES_MAX, ROW_CAND_MAX = 512, 255   # finalize_side, MODE 2 rows: entries of a band's row CSR, candidates of one row (literals there)


# ---- recipes: [kind, seed, n1, n2, keyword arguments] per job (test_cpu_plan.build_jobs) ------------------------------------
def rj(seed, n1, n2, **kw):
    return ["random", seed, n1, n2, kw]


# (what the plan makes of each family at 256 CUs, in a batch of its own: after the semicolon, and asserted through FAMILY_CLAIMS)
FAMILIES = [
    dict(skip_frac=0.0, drop_chain_frac=0.0),                 # pure chains (leaf vs leaf); lean
    dict(skip_frac=0.0, drop_chain_frac=0.0, onehot_frac=1.0),   # ... with one-hot rows throughout: the emission kernel's score table per (symbol, column)
    dict(skip_frac=0.0, drop_chain_frac=0.0, chain_cost_frac=0.2),   # chain-only with costs on some chain edges (lean sweep, R rows per lane)
    dict(skip_frac=0.1, onehot_frac=0.97),                    # almost one-hot: workgroups with and without other rows; narrow, wide workers (40 to 65 nodes, hD 32), crit3 above
    dict(skip_frac=0.2),                                      # merged-graph like skip edges: near window + LDS history; from 40 nodes on crit3 (hD 32), swept by pgm_crit_kernel
    dict(skip_frac=0.3, repeat_frac=0.05),                    # + tandem-repeat edges; crit3 (hD 64)
    dict(skip_frac=0.4, skip_span=3, skip_max=2),             # only near predecessors (distance 2 and 3): the register window alone; narrow (hD 16), at 9 bands crit3 with hDX raised to 8
    dict(skip_frac=0.95, skip_max=9, drop_chain_frac=0.0),    # dense extras: up to 9 far candidates per node, all on chip; no node of the generic path: from 40 nodes on crit3 (nine entries fit the helpers' summary and the row CSR)
    dict(skip_frac=0.1, skip_span=70, repeat_frac=0.03, repeat_span=90),   # far edges: beyond the LDS history and the traceback tile; MODE 2 with remote rows and long columns
    dict(skip_frac=0.25, skip_span=27, skip_max=2),           # distances up to the on-chip limit: deepest history (64 steps), virtual lanes; MODE 2 with remote rows (distances above lane + 16), crit3 jobs swept by pgm_fill_kernel
    # heavy-tailed graphs (MODE 2 with the long / remote entries of the far helpers):
    dict(skip_frac=0.3, skip_span=150, skip_max=5),           # several long edges per node: long slots 7, 6, 5, remote rows, > 3 long: generic
    dict(skip_frac=0.5, skip_span=27, skip_max=14),           # 9-14 on-chip entries per node: overflow table, row CSR
    dict(skip_frac=0.4, skip_span=60, skip_max=10, repeat_frac=0.05, repeat_span=120),   # everything mixed
]
# what every family reaches at 20 and at 61 states, at 256 CUs (its claims), and what it reaches at one of the two only
FAMILY_CLAIMS = [
    ["lean"], ["lean"], ["lean"],
    ["narrow+hD16", "wide+hD32", "crit3+hD32+pgm_crit_kernel", "batch:narrow bands", "batch:wide bands", "batch:wide workers"],
    ["crit3+hD32+pgm_crit_kernel", "batch:crit_c3", "batch:rest_c3"],
    ["crit3+hD64+pgm_crit_kernel"],
    ["narrow+hD16+hDX4"],
    ["crit3+hD32+pgm_crit_kernel", "batch:ncrit", "batch:crit_c3"],
    ["mode2+long1+long2+hD64"],
    ["mode2+long1+hD64", "crit3+hD64+pgm_fill_kernel"],
    ["mode2+long1+long2+generic"],
    ["mode2+long1+ov"],
    ["mode2+long1+long2+ov+generic"],
]
FAMILY_CLAIMS_AT = {(6, 20): ["crit3+hDX->8+pgm_crit_kernel"], (7, 61): ["crit3+hDX->8"], (11, 20): ["mode2+nolong+ov"]}


def family_recipe(fi, dim):
    """test_random_jobs_bit_exact"""
    kw = FAMILIES[fi]
    sizes = [(2, 2), (3, 2), (2, 5), (3, 3), (7, 4), (40, 33), (64, 64), (65, 66), (66, 65), (130, 97), (200, 310), (517, 129)]
    if kw.get("skip_frac", 1) == 0.0:   # chain-only: more than eight bands of 128 / 256 rows (the worker's wavefronts take a second band), ring wrap-around
        sizes = sizes + [(129, 130), (257, 70), (1100, 700), (2500, 90), (90, 2300)]
    if dim == 61:   # the 61-state alphabet (codons): fewer sizes, same families incl. skip and repeat edges
        sizes = [(3, 2), (7, 4), (65, 66), (130, 97), (200, 310)]
    if kw.get("skip_span", 0) >= 60 or kw.get("skip_max", 0) >= 10:   # several bands with remote rows and long columns in flight
        sizes = sizes + [(700, 650)]
    return [rj(1000 + i, n1, n2, dim=dim, **kw) for i, (n1, n2) in enumerate(sizes)]


LARGE_HEAVY_CLAIMS = {0: ["mode2+long1+long2+generic"], 1: ["mode2+long1+ov+generic"], 2: ["mode2+long1+long2+generic"]}
LARGE_HEAVY = [rj(77, 2300, 2200, skip_frac=0.3, skip_span=150, skip_max=5),
               rj(78, 1500, 2600, skip_frac=0.5, skip_span=27, skip_max=14),
               rj(79, 2600, 1400, skip_frac=0.25, skip_span=90, skip_max=6, repeat_frac=0.03, repeat_span=120)]


def crit_wide_recipe(dim):
    """test_critical_path_kernel_and_wide_bands_bit_exact.  At 256 CUs jobs 0 and 2 have remote row entries (a distance above lane + 16
    virtual lanes) and are plain MODE 2 jobs; jobs 1 and 3-6 are crit3 jobs (5 and 6 because the batch does not fill the device and a job
    of 8 bands or more is promoted), but they share the main launch with job 2, so pgm_fill_kernel sweeps them with helpers; job 7
    (5 bands) is the one self-contained sweep on a wide worker.  (pgm_crit_kernel on a job of 20 bands and more: long_job of the wide cases.)"""
    return [rj(7100 + dim, 1500, 1400, dim=dim, skip_frac=0.25, skip_span=27, skip_max=2, drop_chain_frac=0.0),   # 24 bands, hD 64
            rj(7200 + dim, 1300, 700, dim=dim, skip_frac=0.1, skip_span=9, skip_max=3, drop_chain_frac=0.0),    # near and a few far edges, 21 bands
            rj(7300 + dim, 1000, 1100, dim=dim, skip_frac=0.2, skip_span=20, skip_max=2, drop_chain_frac=0.0),
            rj(7400 + dim, 1290, 90, dim=dim, skip_frac=0.5, skip_span=5, skip_max=3, drop_chain_frac=0.0),     # short columns: the sweep is mostly ramp
            rj(7500 + dim, 400, 380, dim=dim, skip_frac=0.2),
            # few far edges, a 32-step history: 8 and 10 bands, promoted to MODE 2 in this batch (crit3)
            rj(7600 + dim, 450, 400, dim=dim, skip_frac=0.03, skip_span=9, skip_max=2, drop_chain_frac=0.0),
            rj(7700 + dim, 600, 300, dim=dim, skip_frac=0.02, skip_span=12, skip_max=2, drop_chain_frac=0.0),
            # ... 5 bands, its chain well below the longest job's: a wide worker of pgm_band_kernel
            rj(7800 + dim, 300, 500, dim=dim, skip_frac=0.04, skip_span=10, skip_max=3, drop_chain_frac=0.0)]


CRIT_WIDE_CLAIMS = (["batch:ncrit", "batch:wide bands", "batch:wide workers"],
                    {0: ["mode2+long1+hD64+list:crit"], 1: ["crit3+hD32+pgm_fill_kernel"], 2: ["mode2+long1+hD64+list:rest"], 3: ["crit3+hDX8+pgm_fill_kernel"],
                     4: ["crit3+pgm_fill_kernel"], 5: ["crit3+pgm_fill_kernel"], 6: ["crit3+pgm_fill_kernel"], 7: ["wide+hD32"]})

# test_job_modes_of_small_and_large_batches_bit_exact: four probes alone, among 22 large fillers, among the 64 fillers of old
PROBES = [rj(8100, 700, 650, skip_frac=0.2, skip_span=20, skip_max=2, drop_chain_frac=0.0),
          rj(8101, 640, 720, skip_frac=0.1, skip_span=9, skip_max=3, drop_chain_frac=0.0),
          rj(8102, 580, 600, skip_frac=0.3, repeat_frac=0.05),
          rj(8103, 900, 300, skip_frac=0.03, skip_span=9, skip_max=2, drop_chain_frac=0.0)]
BIG_FILLERS = [rj(8300 + k, 2000, 2000, skip_frac=0.15, skip_span=12, skip_max=2, drop_chain_frac=0.0) for k in range(22)]
# what the probes reach in each of the three batches
MODES_CLAIMS = {
    "alone": (["batch:promote 0x8"], {0: ["mode2+long1+list:crit+pgm_fill_kernel"], 1: ["crit3+hD32+list:rest+pgm_crit_kernel"], 2: ["crit3+hD64+list:rest+pgm_crit_kernel"],
                                       3: ["crit3+hD32+list:rest+pgm_crit_kernel"]}),
    "big fillers": (["batch:promote 0xffffffff", "batch:crit_c3", "batch:wide workers"],
                    {0: ["mode2+long1+list:rest+pgm_fill_kernel"], 1: ["crit3+hD32+list:rest+pgm_fill_kernel"], 2: ["crit3+hD64+list:rest+pgm_fill_kernel"], 3: ["wide+hD32"],
                     4: ["crit3+list:crit+pgm_crit_kernel"]}),
    "fillers": (["batch:promote 0xffffffff"], {0: ["mode2+long1+list:crit+pgm_fill_kernel"], 1: ["crit3+hD32+list:rest+pgm_crit_kernel"], 2: ["crit3+hD64+list:rest+pgm_crit_kernel"],
                                               3: ["crit3+hD32+list:rest+pgm_crit_kernel"], 4: ["crit3+list:crit+pgm_fill_kernel"]}),
}
FILLERS = [rj(8200 + k, 900, 900, skip_frac=0.15, skip_span=12, skip_max=2, drop_chain_frac=0.0) for k in range(64)]

# test_gpu_dims.py
DIMS = [1, 2, 3, 4, 5, 19, 21, 22, 23, 32, 33, 60, 62, 63, 64]
DIM_SIZES = [(2, 2), (3, 2), (2, 5), (7, 4), (40, 33), (65, 66), (130, 97), (200, 310), (517, 129), (700, 650)]
# pure chains, one-hot rows (in the product form: two sequence graphs, the lean kernel's score table), chains with edge costs,
# skip edges (wide workers, crit3), dense extras (crit3 jobs; no generic node), far edges, heavy-tailed edges (MODE 2 long entries, generic columns)
SWEEP_FAMILIES = {"chain": 0, "onehot": 1, "chaincost": 2, "skip": 4, "dense": 7, "far": 8, "heavy": 10}
# the critical-path kernel's shape: 21, 21 and 7 bands, every predecessor near or in the on-chip history (a small batch: pgm_crit_kernel sweeps both launches)
DIM_CRIT = [(1300, 700, dict(skip_frac=0.1, skip_span=9, skip_max=3, drop_chain_frac=0.0)),
            (1290, 90, dict(skip_frac=0.5, skip_span=5, skip_max=3, drop_chain_frac=0.0)),
            (400, 380, dict(skip_frac=0.2))]


# what each family reaches at every one of DIMS (the seeds, and with them the graphs, differ from size to size)
DIMS_CLAIMS = {"chain": (["lean"], {}), "onehot": (["lean"], {}), "chaincost": (["lean"], {}),
               "skip": (["wide+hD32", "crit3+hD32+pgm_crit_kernel", "batch:wide workers"], {}),
               "dense": (["crit3+hD32+pgm_crit_kernel", "batch:crit_c3"], {}),
               "far": (["mode2+long1+long2+hD64"], {}),
               "heavy": (["mode2+long1+long2+generic", "narrow+hD16"], {}),
               "crit": (["batch:crit_c3", "batch:rest_c3"], {0: ["crit3+hD32+pgm_crit_kernel"], 1: ["crit3+hDX8+pgm_crit_kernel"]})}
NEW_CASES = ["narrow_generic", "wide", "kill_narrow", "kill_wide", "kill_mode2", "kill_crit", "inf_narrow", "inf_wide", "inf_mode2", "inf_crit",
             "chain_broken", "dup"]


def dims_recipe(family, dim):
    """test_align_graphs_every_dim_bit_exact"""
    if family == "crit":
        return [rj(31000 + 100 * dim + i, n1, n2, dim=dim, **kw) for i, (n1, n2, kw) in enumerate(DIM_CRIT)]
    return [rj(30000 + 100 * dim + i, n1, n2, dim=dim, **FAMILIES[SWEEP_FAMILIES[family]]) for i, (n1, n2) in enumerate(DIM_SIZES)]


# ---- the paths no job above reaches -------------------------------------------------------------------------------------------
SMALL = [(40, 33), (65, 66), (130, 97), (200, 310)]   # one band, the 64 / 65 boundary, two and four bands
NEAR = dict(skip_frac=0.3, skip_span=3, skip_max=2)                          # narrow, hD 16
FEW = dict(skip_frac=0.03, skip_span=9, skip_max=2, drop_chain_frac=0.0)      # few far edges, hD 32: wide beside a long job
HUBS = dict(hub_frac=0.03, hub_k=(13, 16), hub_span=16)   # more than PGM_KF8 far candidates: generic in a self-contained sweep, and the hub does not deepen hD


def long_job(dim):
    """a crit job of 24 bands: beside it the chain of a small job's self-contained sweeps ends early enough for a wide worker"""
    return rj(1, 1500, 1400, dim=dim, skip_frac=0.1, skip_span=9, skip_max=3, drop_chain_frac=0.0)


def new_recipes(dim):
    """name -> (recipe, claims, {job: claims of that job}) of the cases added for the paths the older families do not reach"""
    R = {}
    # a: MODE 1 generic nodes in narrow sweeps: hubs in both graphs, then in graph 1 (rows) and in graph 2 (columns) alone
    R["narrow_generic"] = ([rj(50 + i, n1, n2, dim=dim, edit=HUBS, **NEAR) for i, (n1, n2) in enumerate(SMALL)] +
                           [rj(54, 130, 97, dim=dim, edit1=HUBS, **NEAR), rj(55, 200, 310, dim=dim, edit1=HUBS, **NEAR),
                            rj(56, 130, 97, dim=dim, edit2=HUBS, **NEAR), rj(57, 200, 310, dim=dim, edit2=HUBS, **NEAR)],
                           ["narrow+generic+hD16"], {4: ["narrow+generic1"], 5: ["narrow+generic1"], 6: ["narrow+generic2"], 7: ["narrow+generic2"]})
    # b, c: wide workers, with and without generic nodes, two jobs each
    R["wide"] = ([long_job(dim), rj(70, 130, 97, dim=dim, **FEW), rj(71, 300, 500, dim=dim, **FEW),
                  rj(80, 130, 97, dim=dim, edit=dict(HUBS, hub_frac=0.02), **dict(FEW, skip_frac=0.05)),
                  rj(81, 130, 97, dim=dim, edit=dict(HUBS, hub_frac=0.02), **dict(FEW, skip_frac=0.05))],
                 ["batch:wide workers", "batch:wide bands"], {0: ["crit3"], 1: ["wide"], 2: ["wide"], 3: ["wide+generic"], 4: ["wide+generic"]})
    # d: kill nodes
    KILL = dict(kill_frac=0.015, kill_band_edges=True)
    R["kill_narrow"] = ([rj(100 + i, n1, n2, dim=dim, edit=KILL, **NEAR) for i, (n1, n2) in enumerate([(7, 6)] + SMALL)] +
                        [rj(115, 200, 310, dim=dim, edit=dict(HUBS, **KILL), **NEAR)],
                        ["narrow+kill+hD16", "narrow+kill1+kill2", "narrow+kill:row0", "narrow+kill:row63", "narrow+kill:endcol",
                         "narrow+kill+generic"], {})
    R["kill_wide"] = ([long_job(dim), rj(180, 130, 97, dim=dim, edit=KILL, **FEW), rj(181, 300, 500, dim=dim, edit=KILL, **FEW)],
                      ["wide+kill:row0", "wide+kill:row63", "wide+kill:endcol"], {0: ["crit3"], 1: ["wide+kill1+kill2"], 2: ["wide+kill1+kill2"]})
    R["kill_mode2"] = ([rj(110 + i, n1, n2, dim=dim, edit=KILL, **FAMILIES[4]) for i, (n1, n2) in enumerate(SMALL)] +
                       [rj(120 + i, n1, n2, dim=dim, edit=KILL, **FAMILIES[11]) for i, (n1, n2) in enumerate(SMALL[2:])] +
                       [rj(140 + i, n1, n2, dim=dim, edit=KILL, **FAMILIES[10]) for i, (n1, n2) in enumerate(SMALL[1:] + [(700, 650)])],
                       ["mode2+nolong+kill1+kill2", "mode2+long1+long2+kill1+kill2", "mode2+kill:row0", "mode2+kill:row63", "mode2+kill:endcol",
                        "mode2+long+kill:row0", "mode2+long+kill:row63", "mode2+long+kill:endcol", "mode2+kill+generic", "mode2+kill+ov"], {})
    # ... and one kill node in graph 1 / in graph 2 takes a job of the crit kernel's shape off it (its twin without: crit3)
    crit = dict(skip_frac=0.1, skip_span=9, skip_max=3, drop_chain_frac=0.0)
    R["kill_crit"] = ([rj(160, 1300, 700, dim=dim, **crit), rj(160, 1300, 700, dim=dim, edit1=dict(kill_at=[640]), **crit),
                       rj(160, 1300, 700, dim=dim, edit2=dict(kill_at=[-2]), **crit)],
                      [], {0: ["crit3"], 1: ["mode2+nolong+kill1+kill:row0"], 2: ["mode2+nolong+kill2+kill:endcol"]})
    # e: edges of infinite cost
    INF = dict(inf_frac=0.2, inf_chain_frac=0.05)
    inf_all = ["inf:chain>repeat", "inf:chain>regular", "inf:near", "inf:far", "inf:repeat"]
    NEAR4 = dict(skip_frac=0.3, skip_span=4, skip_max=2, repeat_frac=0.05, repeat_span=4)   # ... and far entries and repeat edges at distance 4: still hD 16
    R["inf_narrow"] = ([rj(200 + i, n1, n2, dim=dim, edit=INF, **NEAR4) for i, (n1, n2) in enumerate([(7, 6)] + SMALL)] +
                       [rj(210 + i, n1, n2, dim=dim, edit=INF, **FAMILIES[5]) for i, (n1, n2) in enumerate(SMALL)],
                       ["narrow+" + s for s in inf_all], {})
    R["inf_wide"] = ([long_job(dim), rj(220, 130, 97, dim=dim, edit=INF, repeat_frac=0.05, repeat_span=9, **FEW), rj(221, 300, 500, dim=dim, edit=INF, repeat_frac=0.05, repeat_span=9, **FEW)],
                     ["wide+" + s for s in inf_all], {0: ["crit3"]})
    R["inf_mode2"] = ([rj(230 + i, n1, n2, dim=dim, edit=INF, **FAMILIES[12]) for i, (n1, n2) in enumerate(SMALL[1:] + [(700, 650)])],
                      ["mode2+long+" + s for s in inf_all + ["inf:long"]], {})
    R["inf_crit"] = ([rj(240, 1300, 700, dim=dim, edit=INF, repeat_frac=0.03, repeat_span=9, **crit)], [], {0: ["crit3+" + s for s in inf_all]})
    # f: a pure chain with one infinite chain edge bridged by a skip edge is no lean job; its twin without is
    chain = dict(skip_frac=0.0, drop_chain_frac=0.0)
    R["chain_broken"] = ([rj(250, 65, 66, dim=dim, **chain), rj(250, 65, 66, dim=dim, edit1=dict(broken_chain=[33]), **chain),
                          rj(251, 300, 280, dim=dim, **chain), rj(251, 300, 280, dim=dim, edit2=dict(broken_chain=[64, 200]), **chain)],
                         [], {0: ["lean"], 1: ["narrow+inf:nochain"], 2: ["lean"], 3: ["narrow+inf:nochain"]})
    # g: a repeat edge from the node of a regular edge
    DUP = dict(dup_frac=0.08)
    dup_all = ["dup:d1", "dup:d2", "dup:d3", "dup:far"]
    R["dup"] = ([rj(260 + i, n1, n2, dim=dim, edit=dict(DUP, dup_span=4), **NEAR) for i, (n1, n2) in enumerate(SMALL[1:])] +
                [rj(270 + i, n1, n2, dim=dim, edit=DUP, **FAMILIES[10]) for i, (n1, n2) in enumerate(SMALL[1:])],
                ["narrow+" + s for s in dup_all] + ["mode2+" + s for s in dup_all], {})
    return R


def refusal_recipes(dim):
    """h: the refusals of finalize_side in MODE 2, each on its own: name -> (the job with a hub one entry past the limit, its control
    one entry below).  Chains with hand-placed hubs and one long edge elsewhere (it makes the job a MODE 2 sweep)."""
    chain = dict(skip_frac=0.0, drop_chain_frac=0.0)
    far = [DCAP - 24, DCAP]   # 25 on-chip distances outside the near slots (4 .. 28)
    long_edge = [60, 60, 1, DCAP + 22, DCAP + 22]
    R = {}
    def pair(name, seed, side, hubs_over, hubs_at):
        R[name] = tuple(rj(seed, 260, 200, dim=dim, **dict(chain, **{side: dict(hubs=[long_edge] + h)})) for h in (hubs_over, hubs_at))
    pair("row entries of a band", 300, "edit1", [[80, 81, 200] + far, [100, 100, ROW_ENTRIES_MAX - 400 + 1] + far], [[80, 81, 200] + far, [100, 100, ROW_ENTRIES_MAX - 400] + far])
    pair("remote entries of a band", 301, "edit1", [[220, 220, LIM["PGM_REMOTE_MAX"] + 1, DCAP + 1, DCAP + LIM["PGM_REMOTE_MAX"] + 1]], [[220, 220, LIM["PGM_REMOTE_MAX"], DCAP + 1, DCAP + LIM["PGM_REMOTE_MAX"]]])
    pair("candidates of a row", 302, "edit1", [[100, 100, ROW_CAND_MAX + 1] + far], [[100, 100, ROW_CAND_MAX] + far])
    pair("long entries of a column", 303, "edit2", [[150, 150, LIM["PGM_NLONG"] + 1, DCAP + 12, DCAP + 12 + LIM["PGM_NLONG"]]], [[150, 150, LIM["PGM_NLONG"], DCAP + 12, DCAP + 11 + LIM["PGM_NLONG"]]])
    ring = LIM["PGM_KF8"] + LIM["PGM_OV_ENT"]
    pair("on-chip candidates of a column", 304, "edit2", [[100, 100, ring + 1] + far], [[100, 100, ring] + far])
    over = [LIM["PGM_KF8"] + 1, 4, 4 + LIM["PGM_KF8"]]   # nine on-chip candidates: one entry in the overflow table
    pair("overflow columns", 305, "edit2", [[40, 40 + LIM["PGM_OV_REC"]] + over], [[40, 39 + LIM["PGM_OV_REC"]] + over])
    return R


# ---- reach -----------------------------------------------------------------------------------------------------------------------
def graph_edges(g, v):
    """(from, finite, repeat) of node v in the oracle's order: regular edges, then repeat edges"""
    out = [(int(g.e_col[e]), bool(g.e_val[e] != 0), False) for e in range(g.e_rowptr[v], g.e_rowptr[v + 1])]
    if g.r_rowptr is not None:
        out += [(int(g.r_col[e]), bool(g.r_units[e] != 0), True) for e in range(g.r_rowptr[v], g.r_rowptr[v + 1])]
    return out


def end_is_reachable(g):
    """END from START over edges of finite cost (the oracle, like the reference's own walk, is undefined where it is not)"""
    ok = np.zeros(g.n, bool)
    ok[0] = True
    for v in range(1, g.n):
        ok[v] = any(fin and ok[p] for p, fin, _ in graph_edges(g, v))
    return bool(ok[g.n - 1])


def edge_labels(g, side):
    """labels of one graph from its edge lists alone (flatten_side's place(): the first finite edge from node - 1 takes the chain slot);
    also whether some node has a far candidate (a finite edge outside the chain and near slots)"""
    seen, cand = set(), False
    for v in range(1, g.n):
        edges = graph_edges(g, v)
        if not edges and v < g.n - 1:
            seen.add("kill%d" % side)
            if side == 1 and v % 64 == 0: seen.add("kill:row0")
            if side == 1 and v % 64 == 63: seen.add("kill:row63")
            if side == 2 and v == g.n - 2: seen.add("kill:endcol")
        chain = inf_first = False
        near = set()
        regular = {p for p, _, rep in edges if not rep}
        for p, fin, rep in edges:
            d = v - p
            if rep and p in regular:
                seen.add("dup:d%d" % d if d <= 3 else "dup:far")
            if not fin:
                if rep: seen.add("inf:repeat")
                if d == 1 and not chain: inf_first = True
                elif d <= 3: seen.add("inf:near")
                elif d <= DCAP: seen.add("inf:far")
                else: seen.add("inf:long")
            elif d == 1 and not chain:
                chain = True
                if inf_first: seen.update(["inf:chain", "inf:chain>repeat" if rep else "inf:chain>regular"])
            elif d in (2, 3) and d not in near:
                near.add(d)
            else:
                cand = True
        if inf_first and not chain: seen.add("inf:nochain")
    return seen, cand


def reach(jobs, cus=CUS):
    """(one label set per job, the batch's label set) of the plan of that batch on a device of `cus` CUs"""
    rc, p = TP.plan(jobs, cus)
    assert rc == 0
    h = dict(zip(TP.HEAD, p["head"]))
    bands = np.asarray(p["bands"], np.int64).reshape(-1, 4)   # PgmItem: job, band, priority, count; the narrow bands first
    narrow = set(bands[:h["nbands_narrow"], 0].tolist()) if h["nbands"] else set()
    wide = set(bands[h["nbands_narrow"]:h["nbands"], 0].tolist()) if h["nbands"] else set()
    items = np.asarray(p["items"], np.int64).reshape(-1, 4)
    in_crit, in_rest = set(items[:h["ncrit"], 0].tolist()), set(items[h["ncrit"]:, 0].tolist())
    out = []
    for i, f in enumerate(p["jobs"]):
        j = dict(zip(TP.JOB, f))
        s = set()
        assert (i in in_crit) + (i in in_rest) == (1 if j["mode2"] else 0), i
        if i in in_crit: s.update(["list:crit", "pgm_crit_kernel" if h["crit_c3"] else "pgm_fill_kernel"])
        if i in in_rest: s.update(["list:rest", "pgm_crit_kernel" if h["rest_c3"] else "pgm_fill_kernel"])
        kind = "lean" if j["lean"] else "crit3" if j["crit3"] else "mode2" if j["mode2"] else "wide" if i in wide else "narrow" if i in narrow else None
        assert kind, (i, j)
        assert (i in narrow) + (i in wide) == (kind in ("narrow", "wide")), (i, kind)   # a job is in one list
        s.add(kind)
        l1, c1 = edge_labels(jobs[i].g1, 1)
        l2, c2 = edge_labels(jobs[i].g2, 2)
        s |= l1 | l2
        if j["generic"]:
            s.add("generic")
            if c1 and not c2: s.add("generic1")
            if c2 and not c1: s.add("generic2")
        if j["kill"]: s.add("kill")
        assert bool(j["kill"]) == bool({"kill1", "kill2"} & s)
        if j["nov2"]: s.add("ov")
        if j["long1"]: s.add("long1")
        if j["long2"]: s.add("long2")
        if j["long1"] or j["long2"]: s.add("long")
        if kind == "mode2" and not (j["long1"] or j["long2"]): s.add("nolong")
        if not j["lean"]:
            s.update(["hD%d" % j["hD"], "hDX%d" % j["hDX"]])
        if j["crit3"] and j["hDX"] == 8 and TP.max_onchip_distance(jobs[i].g2) + 1 <= 4: s.add("hDX->8")
        out.append(s)
    b = {"promote %#x" % h["promote_bands"]}
    if h["ncrit"]: b.add("ncrit")
    if h["nbands_narrow"]: b.add("narrow bands")
    if h["nbands"] > h["nbands_narrow"]: b.add("wide bands")
    if h["nwide_workers"]: b.add("wide workers")
    if h["crit_c3"]: b.add("crit_c3")
    if h["rest_c3"]: b.add("rest_c3")
    return out, b


def generic_nodes(jobs, cus=CUS):
    rc, p = TP.plan(jobs, cus)
    assert rc == 0
    return [f[TP.JOB.index("generic")] for f in p["jobs"]]


def missing_claims(jobs, claims, named, cus=CUS):
    """the claims the plan of this batch does not keep: [(claim, job or None)]"""
    per_job, batch = reach(jobs, cus)
    miss = []
    for c in claims:
        if c.startswith("batch:"):
            if c[6:] not in batch: miss.append((c, None))
        elif not any(set(c.split("+")) <= s for s in per_job):
            miss.append((c, None))
    for i, cs in named.items():
        for c in cs:
            if not set(c.split("+")) <= per_job[i]: miss.append((c, i))
    return miss


def build(recipe):
    jobs = TP.build_jobs(recipe)
    for i, j in enumerate(jobs):
        assert end_is_reachable(j.g1) and end_is_reachable(j.g2), "job %d: END is not reachable over finite edges" % i
    return jobs


def check_claims(name, jobs, claims, named, cus):
    """what a GPU test asserts before it creates its batch: on a device with another CU count the plan may send these jobs elsewhere"""
    miss = missing_claims(jobs, claims, named, cus)
    assert not miss, "case %s at %d CUs does not reach %s" % (name, cus, miss)


def gpu_cases():
    """every batch of the GPU parity tests of test_gpu_align.py and test_gpu_dims.py: (name, recipe, claims, claims of named jobs)"""
    for dim in (20, 61):
        for fi in range(len(FAMILIES)):
            yield "family %d D%d" % (fi, dim), family_recipe(fi, dim), FAMILY_CLAIMS[fi] + FAMILY_CLAIMS_AT.get((fi, dim), []), {}
        yield ("crit_wide D%d" % dim, crit_wide_recipe(dim)) + CRIT_WIDE_CLAIMS
    yield "large_heavy", LARGE_HEAVY, [], LARGE_HEAVY_CLAIMS
    for name, fill in (("alone", []), ("big fillers", BIG_FILLERS), ("fillers", FILLERS)):
        yield ("modes " + name, PROBES + fill) + MODES_CLAIMS[name]
    for dim in DIMS:
        for family in sorted(SWEEP_FAMILIES) + ["crit"]:
            yield ("dims %s D%d" % (family, dim), dims_recipe(family, dim)) + DIMS_CLAIMS[family]
    for dim in (20, 61, 4, 64):
        for name, (recipe, claims, named) in new_recipes(dim).items():
            yield "%s D%d" % (name, dim), recipe, claims, named
        yield ("refusals D%d" % dim,) + refusal_case(dim)


def refusal_case(dim):
    """the twelve jobs of refusal_recipes in one batch: every job MODE 2, every first of a pair with a generic node"""
    R = refusal_recipes(dim)
    recipe = [j for pair in R.values() for j in pair]
    named = {}
    for k, name in enumerate(R):
        named[2 * k] = ["mode2+generic"]
        named[2 * k + 1] = ["mode2"]
    return recipe, [], named
