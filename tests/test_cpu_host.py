"""CPU-only checks of the boundary and the host plumbing (no GPU compute calls)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_library_exports_every_declared_symbol():
    """include/pgm_hip.h is the drop-in boundary: every function it declares must be exported by libpgm_hip.so."""
    import prographmsa_amd as pg
    hdr = open(os.path.join(ROOT, "include", "pgm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgm_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 15
    assert sorted(pg.EXPORTS) == declared, (sorted(pg.EXPORTS), declared)
    for name in declared:
        assert hasattr(pg.lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", pg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "not an exported text symbol: " + name


def test_struct_layouts_match_the_header():
    import ctypes as C
    import prographmsa_amd as pg
    assert C.sizeof(pg.pgm_scores) == 40
    assert C.sizeof(pg.pgm_graph) == 8 + 7 * 8
    assert C.sizeof(pg.pgm_align_out) == 16 + 2 * 8
    assert pg.pgm_align_out.map1.offset == 16


def test_cu_shares_never_starve_a_sweep_launch():
    """The CU split of a batch's four sweep launches (pgm_capi.hip cu_shares): every queue with work gets at least one CU, the
    shares never exceed the device, and a launch of the longest chains is only made when it can get a CU.  Covers the
    band-heavy shape that once left the main launch and the longest chains with a grid of zero (round-3 review)."""
    import ctypes as C
    import prographmsa_amd as pg
    out = (C.c_uint32 * 4)()

    def shares(cus, lean, nlean, band, nbands, rest, nrest, ncrit, chain):
        pg.check(pg.lib.pgm_test_cu_shares(cus, lean, nlean, band, nbands, rest, nrest, ncrit, chain, out))
        l, b, c, r = list(out)
        assert l + b + c + r <= max(cus, (nlean > 0) + (nbands > 0) + (nrest > 0)), (l, b, c, r)
        assert (l > 0) == (nlean > 0) and (b > 0) == (nbands > 0) and (r > 0) == (nrest > 0), (l, b, c, r)
        assert c <= ncrit and c <= cus // 2
        return l, b, c, r

    # the headline batch with a fast longest chain (1.8 ms) is bound by throughput: the shares follow the work
    l, b, c, r = shares(256, 64392., 128, 138987., 1579, 226000., 496, 35, 1824.)
    assert c == 35 and l + b + r == 221 and abs(r - 221 * 226000. / 429379.) <= 3, (l, b, c, r)
    # a batch bound by its longest chain: the other launches end early, the main launch keeps the rest
    l, b, c, r = shares(256, 64392., 128, 138987., 1579, 100000., 496, 35, 3300.)
    assert c == 35 and l <= 64392. / (0.6 * 3300.) + 1 and b <= 138987. / (0.75 * 3300.) + 1 and r >= 100
    # band-heavy batch, two MODE 2 jobs on either side of the cut: nobody is left with a grid of zero
    l, b, c, r = shares(256, 0., 0, 2.0e6, 20000, 3000., 40, 25, 900.)
    assert b >= 150 and r >= 1 and c >= 1
    # tiny devices and tiny batches
    for cus in (1, 2, 3, 4, 8):
        shares(cus, 100., 3, 100., 30, 100., 5, 4, 50.)
        shares(cus, 0., 0, 0., 0, 100., 5, 0, 50.)
        shares(cus, 100., 3, 0., 0, 0., 0, 0, 1.)
    assert shares(256, 100., 128, 0., 0, 0., 0, 0, 1.)[0] == 128


def test_no_cpu_fallback_without_a_device():
    """The product path fails loudly when no gfx950 device is present (no oracle / CPU fallback)."""
    import prographmsa_amd as pg
    if pg.lib.pgm_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pg.PgmError):
        pg.Context(0)
    r = subprocess.run([pg.PGMSA_PATH, "--fasta", "--tree", os.path.join(GOLD, "c1.tree"), os.path.join(GOLD, "c1.fa")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "cannot create a context" in r.stderr


def test_product_does_not_link_or_import_the_oracle():
    import prographmsa_amd as pg
    for path in (pg.LIB_PATH, pg.PGMSA_PATH):
        out = subprocess.run(["nm", "-D", path], capture_output=True, text=True).stdout
        assert "pgmo_" not in out
    for dirpath, _, files in os.walk(os.path.join(ROOT, "prographmsa_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", ".inc")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r"import\s+oracle_lib|from\s+oracle_lib|pgmo_[a-z]|#include\s+\".*oracle|libpgm_oracle", txt), f


def test_job_dump_roundtrip_and_oracle_invariants(oracle_build, tmp_path):
    """pgmsa --dump_jobs -> jobs.load_jobs -> oracle: mappings are monotone, cover every node once, start/end right."""
    import oracle_lib
    from prographmsa_amd import jobs as J
    dump = str(tmp_path / "jobs.bin")
    subprocess.run([os.path.join(oracle_build, "pgmsa_oracle"), "--fasta", "--tree", os.path.join(GOLD, "c1.tree"),
                    "--dump_jobs", dump, os.path.join(GOLD, "c1.fa")], check=True, capture_output=True)
    js = J.load_jobs(dump)
    assert len(js) == 7
    for j in js:
        r = oracle_lib.align_graphs(j)
        m1, m2 = r["map1"], r["map2"]
        assert r["status"] == 0 and len(m1) == len(m2)
        assert (m1[0], m2[0]) == (0, 0) and (m1[-1], m2[-1]) == (j.g1.n - 1, j.g2.n - 1)
        for m in (m1, m2):
            v = m[m != 0xFFFFFFFF].astype(np.int64)
            assert np.all(np.diff(v) > 0)
        assert not np.any((m1 == 0xFFFFFFFF) & (m2 == 0xFFFFFFFF))


@pytest.mark.parametrize("case,flags,gold", [("c1.fa", ["-a", "-m", "-T", "-i", "0"], "c1.nw_ml.tree"), ("c2.fa", ["-a", "-m", "-T", "-i", "0"], "c2.nw_ml.tree")])
def test_all_pairs_farm_one_vs_k_workers(oracle_build, case, flags, gold):
    """computePwDistances (host/distance.cpp) farms the alignPair tiles to one host thread per device context through an
    atomic tile counter.  Same work queue with 1, 2, 3 and 5 workers and three tile sizes (oracle backend on the CPU; the
    product binds the same code to one pgm_ctx per GPU): identical newick, identical to the reference binary's."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    want = open(os.path.join(GOLD, gold)).read()
    seen = set()
    for workers, tile in ((1, 100000), (2, 7), (3, 5), (5, 64)):
        env = dict(os.environ, PGM_FARM_WORKERS=str(workers), PGM_NW_TILE=str(tile))
        r = subprocess.run([exe] + flags + ["--stats", os.path.join(GOLD, case)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (workers, tile)
        st = [ln for ln in r.stderr.splitlines() if ln.startswith('{"backend"')][-1]
        assert '"farm_workers": %d' % workers in st
        seen.add(r.stdout)
    assert len(seen) == 1


@pytest.mark.parametrize("case,flags,gold", [("c2.fa", ["--fasta", "-t", os.path.join(GOLD, "c2.tree")], None),
                                             ("c1.fa", ["--fasta", "-t", os.path.join(GOLD, "c1.tree"), "--cs_profile", os.path.join(GOLD, "K50.lib")], "c1.cs.out.fa"),
                                             ("c1.fa", ["--fasta", "-a"], "c1.a_iter.out.fa")])
def test_level_and_leaf_farm_one_vs_k_workers(oracle_build, case, flags, gold):
    """The jobs of a guide-tree level (alignGraphsBatch), the leaves' context profiles and the merges of a level are dealt to
    the device contexts (farm_shards: by cost, longest first; one host thread per context: host/host_threads.cpp; the
    callers are host/graph_align.cpp and host/progressive.cpp).  1, 2, 3 and 5 workers over the oracle backend: identical FASTA, identical to the reference's."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    outs = {}
    for workers in (1, 2, 3, 5):
        env = dict(os.environ, PGM_FARM_WORKERS=str(workers))
        r = subprocess.run([exe] + flags + ["--stats", os.path.join(GOLD, case)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        st = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith('{"backend"')][-1])
        assert st["farm_level_workers"] == min(workers, 32 if case == "c2.fa" else 4)
        if "--cs_profile" in flags:
            assert st["farm_leaf_workers"] == workers
        outs[workers] = r.stdout
    assert len(set(outs.values())) == 1
    if gold:
        assert outs[1] == open(os.path.join(GOLD, gold)).read()


@pytest.mark.parametrize("case,flags,gold", [("c2.fa", ["--fasta", "-t", os.path.join(GOLD, "c2.tree")], "c2.out.fa"),
                                             ("c1.fa", ["--fasta", "-t", os.path.join(GOLD, "c1.tree"), "--cs_profile", os.path.join(GOLD, "K50.lib")], "c1.cs.out.fa"),
                                             ("c1.fa", ["--fasta", "-a"], "c1.a_iter.out.fa"),
                                             ("cd1.fa", ["--codon", "--fasta", "-t", os.path.join(GOLD, "cd1.tree")], "cd1.out.fa")])
def test_resident_pass_sharded_by_subtree(oracle_build, case, flags, gold):
    """A pass whose profiles never leave the devices, on several of them (host/progressive.cpp assign_owners): the guide tree is cut into
    three subtrees per worker, every node of a subtree lives on its worker (leaves built there, jobs and merges run there), a node above
    the cut on the worker of its larger child, and the other child's matrix is copied over once (Backend::resident_import).  The oracle
    backend plays the devices with one arena of host memory per worker and refuses a matrix used on a worker that does not hold it.
    1, 2, 3 and 5 workers: identical FASTA, the reference's; resident, with copies only where the tree is cut."""
    exe = os.path.join(oracle_build, "pgmsa_oracle")
    for workers in (1, 2, 3, 5):
        env = dict(os.environ, PGM_FARM_WORKERS=str(workers), PGM_ORACLE_RESIDENT="1")
        r = subprocess.run([exe] + flags + ["--stats", os.path.join(GOLD, case)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        st = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith('{"backend"')][-1])
        assert st["resident"] is True
        nseq = open(os.path.join(GOLD, case)).read().count(">")
        if workers == 1:
            assert st["resident_imports"] == 0
        else:
            assert 0 < st["resident_imports"] <= min(3 * workers, nseq) - 1   # at most one copy per node above the cut
            assert st["farm_level_workers"] == min(workers, nseq // 2)
        assert r.stdout == open(os.path.join(GOLD, gold)).read(), workers


def test_farm_shards_cover_every_unit_once():
    """farm_shards is exercised through the driver above; its contract (every unit in exactly one shard, longest first, least
    loaded worker) is restated here on the Python twin that bench.py uses for the process-per-GPU launch."""
    from prographmsa_amd import farm
    for world in (1, 2, 3, 5, 8):
        sh = farm.lpt_shards([7.0, 7.0, 3.0, 9.0, 1.0, 1.0, 4.0, 12.0, 5.0], world)
        assert sorted(i for s_ in sh for i in s_) == list(range(9))


def test_random_job_generator_is_deterministic():
    from prographmsa_amd import jobs as J
    a, b = J.random_job(5, 30, 40, skip_frac=0.3, repeat_frac=0.1), J.random_job(5, 30, 40, skip_frac=0.3, repeat_frac=0.1)
    assert np.array_equal(a.g1.e_col, b.g1.e_col) and np.array_equal(a.g2.sites, b.g2.sites)
    assert a.g1.r_col is not None or a.g2.r_col is not None


def test_farm_partitions():
    from prographmsa_amd import farm
    lengths = [5, 9, 2, 7, 7, 3, 11]
    pairs = farm.sorted_pairs(lengths)
    assert sorted(pairs) == farm.all_pairs(len(lengths))
    cost = [lengths[a] * lengths[b] for a, b in pairs]
    assert cost == sorted(cost, reverse=True)
    assert farm.tile_size(32640, 1) == 10880 and farm.tile_size(32640, 8) == 1360 and farm.tile_size(100, 8) == 256 and farm.tile_size(100, 8, "7") == 7
    q = farm.TicketQueue("t", 1)
    assert [q.next() for _ in range(4)] == [0, 1, 2, 3]
    for world in (1, 2, 3, 8):
        sh = farm.lpt_shards([9.0, 1.0, 4.0, 4.0, 2.0, 7.0, 3.0], world)
        assert sorted(i for s_ in sh for i in s_) == list(range(7))
        loads = [sum([9.0, 1.0, 4.0, 4.0, 2.0, 7.0, 3.0][i] for i in s_) for s_ in sh]
        assert max(loads) <= 30.0 / world + 9.0
        spans = [farm.shard_range(13, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == 13 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
