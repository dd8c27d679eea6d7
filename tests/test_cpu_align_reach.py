"""The GPU parity tests of alignGraphs hold what they claim: every batch of test_gpu_align.py and test_gpu_dims.py (align_cases.py),
planned on the host for 256 CUs (the MI355X) through pgm_test_batch_plan, sends its jobs to the sweeps, launches and node paths the
case names, and all of them together reach every path on the list below.  A planning constant that moves a job off the kernel it was
written for fails here, by the case's name, instead of leaving the suite green and testing less."""
import pytest

import align_cases as A

CASES = list(A.gpu_cases())

# One job, run by a GPU parity test, with all the labels of a line.
REQUIRED = [
    # the sweeps the suite reached before the cases of new_recipes
    "lean", "narrow", "wide", "crit3+pgm_crit_kernel", "crit3+pgm_fill_kernel", "crit3+hDX->8", "crit3+list:crit+pgm_crit_kernel", "crit3+list:rest+pgm_crit_kernel",
    "mode2+nolong", "mode2+long1", "mode2+long2", "mode2+ov", "mode2+generic", "mode2+list:crit", "mode2+list:rest",
    # a: generic nodes of a self-contained sweep, rows and columns; b, c: wide workers
    "narrow+generic1", "narrow+generic2", "wide+generic",
    # d: kill nodes
    "narrow+kill1", "narrow+kill2", "narrow+kill:row0", "narrow+kill:row63", "narrow+kill:endcol", "narrow+kill+generic",
    "wide+kill1", "wide+kill2", "wide+kill:row0", "wide+kill:row63", "wide+kill:endcol",
    "mode2+nolong+kill1", "mode2+nolong+kill2", "mode2+nolong+kill:row0", "mode2+nolong+kill:row63", "mode2+nolong+kill:endcol",
    "mode2+long+kill1", "mode2+long+kill2", "mode2+long+kill:row0", "mode2+long+kill:row63", "mode2+long+kill:endcol", "mode2+kill+generic", "mode2+kill+ov",
    # e: edges of infinite cost
] + [kind + "+" + e for kind in ("narrow", "wide", "mode2", "crit3+pgm_crit_kernel")
     for e in ("inf:chain>repeat", "inf:chain>regular", "inf:near", "inf:far", "inf:repeat")] + [
    "mode2+inf:long",
    # f: a chain with an infinite chain edge
    "narrow+inf:nochain",
    # g: two edges from one predecessor
] + [kind + "+" + d for kind in ("narrow", "mode2") for d in ("dup:d1", "dup:d2", "dup:d3", "dup:far")]
REQUIRED_BATCH = ["ncrit", "narrow bands", "wide bands", "wide workers", "promote 0x8", "promote 0xffffffff", "crit_c3", "rest_c3"]


@pytest.fixture(scope="module")
def reached():
    """name -> (jobs, per-job labels, batch labels) of every case at 256 CUs, planned once"""
    out = {}
    for name, recipe, claims, named in CASES:
        jobs = A.build(recipe)
        out[name] = (jobs,) + A.reach(jobs, A.CUS)
    return out


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_reaches_what_it_claims(reached, case):
    name, recipe, claims, named = case
    jobs, per_job, batch = reached[name]
    miss = []
    for c in claims:
        if c.startswith("batch:"):
            if c[6:] not in batch: miss.append(c)
        elif not any(set(c.split("+")) <= s for s in per_job):
            miss.append(c)
    for i, cs in named.items():
        miss += ["job %d: %s" % (i, c) for c in cs if not set(c.split("+")) <= per_job[i]]
    assert not miss, "%s does not reach %s at %d CUs" % (name, miss, A.CUS)
    assert miss == ["job %s: %s" % (i, c) if i is not None else c for c, i in A.missing_claims(jobs, claims, named, A.CUS)]   # (what the GPU tests call)


def test_cases_reach_every_path_together(reached):
    """No label is satisfied by a job that no GPU test runs: `reached` holds the GPU tests' batches and nothing else."""
    jobs_labels = [s for _, per_job, _ in reached.values() for s in per_job]
    batch_labels = set().union(*[b for _, _, b in reached.values()])
    miss = [c for c in REQUIRED if not any(set(c.split("+")) <= s for s in jobs_labels)] + ["batch:" + c for c in REQUIRED_BATCH if c not in batch_labels]
    assert not miss, miss


def test_every_claim_names_known_labels():
    """a misspelt label can never be reached; one that nothing claims or requires is dead"""
    known = set((
        "lean narrow wide mode2 crit3 list:crit list:rest pgm_crit_kernel pgm_fill_kernel generic generic1 generic2 kill kill1 kill2 ov long1 long2 long nolong "
        "hD16 hD32 hD64 hDX4 hDX8 hDX16 hDX32 hDX->8 kill:row0 kill:row63 kill:endcol inf:chain inf:chain>repeat inf:chain>regular inf:nochain inf:near inf:far "
        "inf:long inf:repeat dup:d1 dup:d2 dup:d3 dup:far").split())
    for name, recipe, claims, named in CASES:
        for c in claims + [c for cs in named.values() for c in cs]:
            if c.startswith("batch:"):
                assert c[6:] in REQUIRED_BATCH, (name, c)
            else:
                assert set(c.split("+")) <= known, (name, c)
    for c in REQUIRED:
        assert set(c.split("+")) <= known, c


def test_refusals_of_a_mode2_sweep_each_on_their_own():
    """Each rule by which finalize_side sends a node of a MODE 2 job to the generic path, crossed by one entry: the job with the hub one
    entry past the limit has a generic node, its control with the hub at the limit has none (the plan reports only the count)."""
    R = A.refusal_recipes(20)
    assert sorted(R) == sorted(["row entries of a band", "remote entries of a band", "candidates of a row", "long entries of a column",
                                "on-chip candidates of a column", "overflow columns"])
    for name, pair in R.items():
        over, at = A.generic_nodes(A.build(list(pair)), A.CUS)
        assert (over, at) == (1, 0), (name, over, at)
    # the limits the hubs are placed against are those of pgm_device.h and of finalize_side
    text = open(A.os.path.join(A.ROOT, "prographmsa_amd", "csrc", "pgm_plan.h")).read()
    assert "band_entries + nc > %du" % A.ROW_ENTRIES_MAX in text and "nc > %du" % A.ROW_CAND_MAX in text


def test_probes_take_other_routes_among_the_big_fillers(reached):
    """test_job_modes_of_small_and_large_batches_bit_exact: what differs for the four probes between the batches.  Alone and among the 64
    fillers of 900 x 900 nothing that selects device code differs (only the lists' order and the workers); among 22 fillers of
    2000 x 2000 probes 1 and 2 are swept by pgm_fill_kernel instead of pgm_crit_kernel and probe 3 by a wide worker of pgm_band_kernel."""
    sel = {"lean", "narrow", "wide", "mode2", "crit3", "pgm_crit_kernel", "pgm_fill_kernel", "long1", "long2", "ov", "generic"}
    alone, big, old = [[s & sel for s in reached["modes " + k][1][:4]] for k in ("alone", "big fillers", "fillers")]
    assert alone == old
    assert alone[0] == big[0] == {"mode2", "long1", "pgm_fill_kernel"}
    for i in (1, 2):
        assert alone[i] == {"crit3", "pgm_crit_kernel"} and big[i] == {"crit3", "pgm_fill_kernel"}
    assert alone[3] == {"crit3", "pgm_crit_kernel"} and big[3] == {"wide"}


def test_edits_off_leave_the_generator_alone():
    """random_job without edit options is the job of the same seed before there were any: no draw from its stream (test_cpu_plan's
    fixtures pin the plans of such jobs); with them, the unedited graph is the one the edges were added to."""
    import numpy as np
    from prographmsa_amd import jobs as J
    a = J.random_job(5, 90, 80, skip_frac=0.3, repeat_frac=0.05)
    b = J.random_job(5, 90, 80, skip_frac=0.3, repeat_frac=0.05, edit=dict(), edit1=None)
    c = J.random_job(5, 90, 80, skip_frac=0.3, repeat_frac=0.05, edit1=dict(kill_at=[40]))
    for x, y in ((a.g1, b.g1), (a.g2, b.g2), (a.g2, c.g2)):
        for f in ("sites", "e_rowptr", "e_col", "e_val", "r_rowptr", "r_col", "r_units"):
            assert np.array_equal(getattr(x, f), getattr(y, f)), f
    assert np.array_equal(a.M, c.M) and np.array_equal(a.scores, c.scores) and np.array_equal(a.g1.sites, c.g1.sites)
    assert c.g1.e_rowptr[41] == c.g1.e_rowptr[40] and 39 in c.g1.e_col[c.g1.e_rowptr[41]:c.g1.e_rowptr[42]]


def test_end_is_reachable_check():
    from prographmsa_amd import jobs as J
    j = J.random_job(6, 30, 28, skip_frac=0.0, drop_chain_frac=0.0)
    assert A.end_is_reachable(j.g1)
    j.g1.e_val[10] = 0.0   # the only edge of a node of a chain at infinite cost
    assert not A.end_is_reachable(j.g1)
