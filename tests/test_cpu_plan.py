"""The host-only planning of an align batch (csrc/pgm_plan.h) through pgm_test_batch_plan: the sweep every job gets, the LDS layout of
its sweeping wavefront, the work lists, their order and the workers of every launch are exactly what the commit before the planning
was split out of pgm_align_batch_create_res computed.

Fixtures tests/golden/plan_*.json: recorded from that parent commit, not from the code under test — a temporary patch at the end of
its pgm_align_batch_create_res wrote the fields below for every batch (one run on an MI355X, the old function needs a device; an
environment variable stood in for the device's CU count).  A fixture holds the recipe of its jobs (prographmsa_amd.jobs: random_job,
sequence_job, both deterministic) and one plan per CU count; a batch of headline size stores a SHA-256 of each packed list instead
of the list."""
import ctypes as C
import glob
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CUS = (256, 1, 4, 8, 64)
HEAD = ("dp", "promote_bands", "nitems", "ncrit", "nbands", "nbands_narrow", "nlean", "ntb", "ntb_c", "ntb_b", "nworkers", "nlean_workers",
        "nband_workers", "nwide_workers", "ncrit_workers", "ntb_workers", "ntb_b_workers", "crit_c3", "rest_c3", "rest_cus", "narrow_bands",
        "rest_items", "crit_items")
JOB = ("lean", "has_extras", "mode2", "hD", "hDX", "slot_bytes", "aux_off", "ov_off", "rh_off", "c3_off", "nov2", "has_far", "long1", "long2",
       "crit3", "far_slack", "nslots", "generic", "kill")
LISTS = ("items", "bands", "lean_list", "tblist")


def build_jobs(recipe):
    """recipe: [kind, seed, n1 | L1, n2 | L2, keyword arguments] per job"""
    from prographmsa_amd import jobs as J
    out = []
    for kind, seed, a, b, kw in recipe:
        kw = dict(kw)
        kill = kw.pop("kill_nodes", ())   # interior nodes of graph 1 that lose every predecessor (random_graph always leaves one)
        job = (J.random_job if kind == "random" else J.sequence_job)(seed, a, b, **kw)
        g = job.g1
        for v in kill:
            lo, hi = int(g.e_rowptr[v]), int(g.e_rowptr[v + 1])
            g.e_col, g.e_val = np.delete(g.e_col, np.s_[lo:hi]), np.delete(g.e_val, np.s_[lo:hi])
            g.e_rowptr[v + 1:] -= hi - lo
        out.append(job)
    return out


def site_refs(jobs, dev_sites):
    """Resident profiles for side 1 of every job: dev_sites(bytes) -> address of the matrix (the plan never dereferences it), a
    node -> column map into a matrix of n + 3 columns."""
    import prographmsa_amd as pg
    refs, keep = (pg.pgm_site_ref * len(jobs))(), []
    for i, j in enumerate(jobs):
        ncols = j.g1.n + 3
        nmap = ((np.arange(j.g1.n, dtype=np.uint64) * 7) % ncols).astype(np.uint32)
        keep.append(nmap)
        refs[i].dev_sites = C.cast(dev_sites(8 * ncols * j.g1.dim), C.POINTER(C.c_double))
        refs[i].node_map = nmap.ctypes.data_as(C.POINTER(C.c_uint32))
        refs[i].ncols = ncols
    return refs, keep


def plan(jobs, cus, res1=None, flags=0):
    """pgm_test_batch_plan -> (return code, plan as the fixtures store it)"""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J
    cj = J.CJobs(jobs)
    nbands = max(1, sum((j.g1.n - 1 + 63) // 64 for j in jobs if j.g1.n >= 2))
    head, dhead = np.zeros(len(HEAD), np.uint32), np.zeros(9, np.float64)
    fields = np.zeros((max(1, cj.n), len(JOB)), np.uint32)
    items, bands = np.zeros(4 * nbands, np.uint32), np.zeros(4 * nbands, np.uint32)
    lean, tbl = np.zeros(max(1, cj.n), np.uint32), np.zeros(2 * max(1, cj.n), np.int32)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = pg.lib.pgm_test_batch_plan(cj.n, cj.g1, cj.g2, cj.m, cj.sc, flags, res1, None, cus, u32(head), dhead.ctypes.data_as(C.POINTER(C.c_double)),
                                    u32(fields), u32(items), u32(bands), u32(lean), tbl.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != pg.PGM_OK:
        return rc, None
    h = dict(zip(HEAD, head.tolist()))
    return rc, {"head": head.tolist(), "dhead": [float(x).hex() for x in dhead], "jobs": fields[:cj.n].tolist(),
                "items": items[:4 * h["nitems"]].tolist(), "bands": bands[:4 * h["nbands"]].tolist(), "lean_list": lean[:h["nlean"]].tolist(),
                "tblist": tbl[:2 * (h["ntb"] + h["ntb_c"] + h["ntb_b"])].tolist()}


def digest(p):
    """the lists of a plan as SHA-256 of their packed 32-bit words"""
    q = dict(p)
    for k in LISTS:
        q[k] = hashlib.sha256(np.asarray(p[k], np.int32 if k == "tblist" else np.uint32).tobytes()).hexdigest()
    return q


def fixtures():
    return sorted(glob.glob(os.path.join(GOLD, "plan_*.json")))


def max_onchip_distance(g):
    """flatten_side's maxd_cap: the largest distance <= 28 of a finite edge outside the chain slot (>= 1)"""
    best = 1
    for v in range(g.n):
        chain = False
        edges = [(int(g.e_col[e]), g.e_val[e] != 0) for e in range(g.e_rowptr[v], g.e_rowptr[v + 1])]
        if g.r_rowptr is not None:
            edges += [(int(g.r_col[e]), g.r_units[e] != 0) for e in range(g.r_rowptr[v], g.r_rowptr[v + 1])]
        for frm, finite in edges:
            if not finite:
                continue
            if v - frm == 1 and not chain:
                chain = True
            elif v - frm <= 28:
                best = max(best, v - frm)
    return best


@pytest.mark.parametrize("path", fixtures(), ids=lambda p: os.path.basename(p)[5:-5])
def test_plan_equals_the_parent_commit(path):
    fx = json.load(open(path))
    jobs = build_jobs(fx["jobs"])
    scratch = np.zeros(1, np.float64)
    res1, keep = site_refs(jobs, lambda nbytes: scratch.ctypes.data) if fx["resident"] else (None, None)
    assert sorted(fx["plans"]) == sorted(str(c) for c in CUS)
    for cus in CUS:
        rc, p = plan(jobs, cus, res1)
        assert rc == 0
        want = fx["plans"][str(cus)]
        got = digest(p) if fx["digest"] else p
        for k in ("head", "dhead", "jobs") + LISTS:
            assert got[k] == want[k], (os.path.basename(path), cus, k)


def test_fixtures_cover_every_branch_of_the_plan():
    """A fixture that stopped reaching a branch fails here instead of passing quietly."""
    seen = set()
    for path in fixtures():
        fx = json.load(open(path))
        jobs = build_jobs(fx["jobs"]) if any(j[JOB.index("crit3")] for p in fx["plans"].values() for j in p["jobs"]) else None
        seen.add("resident" if fx["resident"] else "own profiles")
        for p in fx["plans"].values():
            h = dict(zip(HEAD, p["head"]))
            if not fx["jobs"]:
                seen.add("njobs == 0")
            seen.add("tier %d" % h["dp"])
            seen.add("promote_bands %#x" % h["promote_bands"])
            if h["nbands_narrow"]: seen.add("narrow band")
            if h["nbands"] > h["nbands_narrow"]: seen.add("wide band")
            if h["nbands_narrow"] and h["nwide_workers"]: seen.add("narrow and wide workers")
            if h["ncrit"]: seen.add("ncrit > 0")
            if h["nitems"] and not h["ncrit"]: seen.add("items without ncrit")
            for i, f in enumerate(p["jobs"]):
                j = dict(zip(JOB, f))
                if j["lean"]: seen.add("lean")
                if j["mode2"] and not j["crit3"]: seen.add("mode2 without crit3")
                if j["crit3"]: seen.add("crit3")
                if j["crit3"] and j["hDX"] == 8 and max_onchip_distance(jobs[i].g2) + 1 <= 4: seen.add("crit3 with hDX raised to 8")
                if j["long1"] or j["long2"]: seen.add("long")
                if j["nov2"]: seen.add("nov2 > 0")
                if j["generic"]: seen.add("generic node")
                if j["kill"]: seen.add("kill node")
    want = {"lean", "narrow band", "wide band", "mode2 without crit3", "crit3", "crit3 with hDX raised to 8", "long", "nov2 > 0", "generic node", "kill node",
            "promote_bands 0x8", "promote_bands 0xffffffff", "ncrit > 0", "items without ncrit", "narrow and wide workers", "tier 4", "tier 20", "tier 64",
            "resident", "njobs == 0"}
    assert want <= seen, sorted(want - seen)


def test_invalid_input_returns_what_create_returns():
    """PGM_ERR_INVALID with the job's index in the message, as pgm_align_batch_create_res answers the same input."""
    import prographmsa_amd as pg
    from prographmsa_amd import jobs as J

    def fails(jobs, message, res1=None, mangle=None):
        cj = J.CJobs(jobs)
        if mangle:
            mangle(cj)
        buf = (C.c_uint32 * 4096)()
        d = (C.c_double * 9)()
        rc = pg.lib.pgm_test_batch_plan(cj.n, cj.g1, cj.g2, cj.m, cj.sc, 0, res1, None, 256, buf, d, buf, buf, buf, buf, C.cast(buf, C.POINTER(C.c_int32)))
        assert rc == pg.PGM_ERR_INVALID and pg.lib.pgm_last_error().decode() == message, (rc, pg.lib.pgm_last_error())

    good = lambda seed: J.random_job(seed, 40, 50)
    assert pg.lib.pgm_test_batch_plan(1, None, None, None, None, 0, None, None, 256, None, None, None, None, None, None, None) == pg.PGM_ERR_INVALID
    assert pg.lib.pgm_last_error().decode() == "null argument"

    def null_graph(cj): cj.g1[1] = C.POINTER(pg.pgm_graph)()
    fails([good(1), good(2)], "invalid job 1", mangle=null_graph)
    def other_dim(cj): cj._g2[1].dim = 19
    fails([good(1), good(2)], "invalid job 1", mangle=other_dim)
    def one_node(cj): cj._g1[0].n = 1
    fails([good(1), good(2)], "invalid job 0", mangle=one_node)
    forward = good(3)
    forward.g2.e_col[forward.g2.e_rowptr[7]] = 9   # an edge of node 7 from node 9
    fails([good(1), good(2), forward], "invalid graph in job 2")
    jobs = [good(1), good(2)]
    res1, keep = site_refs(jobs, lambda nbytes: 64)
    keep[1][5] = jobs[1].g1.n + 3   # one past the last column
    fails(jobs, "invalid graph in job 1", res1=res1)


def test_plan_header_is_host_only(tmp_path):
    """pgm_plan.h needs no kernel header and no HIP runtime: a translation unit of it alone compiles and runs with the host compiler."""
    src = tmp_path / "plan_only.cpp"
    src.write_text('#include "pgm_plan.h"\nint main() { std::vector<PgmJob> none; return plan_schedule(none, {}, 4u).nworkers == 1u ? 0 : 1; }\n')
    exe = str(tmp_path / "plan_only")
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", os.path.join(ROOT, "prographmsa_amd", "csrc"), "-o", exe, str(src)], check=True)
    assert subprocess.run([exe]).returncode == 0
    text = open(os.path.join(ROOT, "prographmsa_amd", "csrc", "pgm_plan.h")).read()
    includes = [ln for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and not any("_kernels.h" in ln or "hip_runtime" in ln for ln in includes), includes
