"""The command-line driver (host/main.cpp and the driver_*.cpp files) as a black box, through the CPU oracle driver.

The solo run is the loop of a `--batch` chunk on a list of one family (host/driver_family.cpp).  CASES pins the driver to commit
8881cb7, the last one whose solo run had a loop of its own: for every command line of the table the output files, every byte on
stdout, every message on stderr (the `--stats` line aside: it holds times), the exit code and the keys of the `--stats` line in
their order are what that commit gives.  EXPECTED was recorded with the `pgmsa_oracle` built from 8881cb7 (record() below, run on
that binary), never with the code under test.  The --ml_tree and --bootstrap files hold numbers printed at full precision: their
md5s are those of the build container's libm.

Beside the table: `-T` with --bootstrap and --ml_tree together writes what the two write alone (the final alignment is computed
once for both), every refusal of the option parser that no other test asserts, with its exact message, and the oracle's Makefile
rebuilds after a change to an included file."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import batch_util as bu
import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# name -> arguments ({G}: tests/golden, {T}: the case's own directory, where inputs() puts r.fa / r.trd / b.list)
CASES = {
    "default_c1": ["--fasta", "{G}/c1.fa"],
    "default_c2": ["--fasta", "{G}/c2.fa"],
    "i3": ["--fasta", "-i", "3", "{G}/c1.fa"],
    "t": ["--fasta", "-t", "{G}/c1.tree", "{G}/c1.fa"],
    "topology": ["--fasta", "--topology", "{G}/c1.tree", "{G}/c1.fa"],
    "T": ["-T", "{G}/c1.fa"],
    "T_bootstrap_ml_tree": ["-T", "--bootstrap", "4", "--bootstrap_out", "{T}/b.nwk", "--ml_tree", "{T}/m.nwk", "{G}/c1.fa"],
    "r": ["--fasta", "-r", "{G}/c1.fa"],
    "rr": ["--fasta", "-rr", "{G}/c1.fa"],
    "W": ["--fasta", "-W", "{G}/c1.fa"],
    "R_read_repeats": ["--fasta", "-R", "--read_repeats", "{T}/r.trd", "{T}/r.fa"],
    "profile_out": ["--fasta", "--profile_out", "{T}/p.prof", "-t", "{G}/a1.tree", "{G}/a1.fa"],
    "profile_out_iterations": ["--fasta", "--profile_out", "{T}/p.prof", "{G}/c1.fa"],
    "cs_profile": ["--fasta", "-c", "{G}/K50.lib", "{G}/c1.fa"],
    "codon": ["--codon", "--fasta", "{G}/cd1.fa"],
    "ancestral_seqs": ["--fasta", "--ancestral_seqs", "{G}/c1.fa"],
    "early_refinement": ["--fasta", "--early_refinement", "{G}/c1.fa"],
    "guidance": ["--fasta", "--guidance", "3", "--guidance_out", "{T}/g.txt", "--guidance_residues", "{T}/g.res", "--guidance_dump", "{T}/gd", "{G}/c1.fa"],
    "bootstrap": ["--fasta", "--bootstrap", "5", "--bootstrap_out", "{T}/b.nwk", "--bootstrap_tbe", "{T}/b.tbe", "--bootstrap_trees", "{T}/b.trees",
                  "--bootstrap_taxa", "{T}/b.taxa", "--bootstrap_taxa_edges", "{T}/b.edges", "{G}/c1.fa"],
    "ml_gamma": ["--fasta", "--ml_tree", "{T}/m.nwk", "--ml_sites", "{T}/m.sites", "--ml_gamma", "4", "--ml_rates", "{T}/m.rates", "{G}/c1.fa"],
    "batch": ["--fasta", "--batch", "{T}/b.list"],
}
INPUTS = ("r.fa", "r.trd", "b.list")


def inputs(d):
    """The inputs the table does not find under tests/golden: a family with tandem repeats and its T-REKS report, and a list of
    three families whose second line names a file that does not exist."""
    seqs, trd = gen.gen_repeat_family(8, 60, 22)
    with open(os.path.join(d, "r.fa"), "w") as f:
        f.write(gen.fasta(seqs))
    with open(os.path.join(d, "r.trd"), "w") as f:
        f.write(trd)
    with open(os.path.join(d, "b.list"), "w") as f:
        f.write("%s/c1.fa\t%s/o1.fa\n%s/missing.fa\t%s/o2.fa\n%s/a1.fa\t%s/o3.fa\t%s/a1.tree\n" % (GOLD, d, d, d, GOLD, d, GOLD))


def md5(b):
    return hashlib.md5(b).hexdigest()


def record(exe, name, d):
    """One command line of the table with --stats in a directory of its own: what EXPECTED holds for it."""
    d = str(d)
    inputs(d)
    args = [x.replace("{G}", GOLD).replace("{T}", d) for x in CASES[name]]
    r = subprocess.run([exe, "--stats"] + args, capture_output=True, timeout=300)
    err = r.stderr.decode().replace(GOLD, "{G}").replace(d, "{T}").splitlines(True)
    stats = [l for l in err if l.startswith('{"backend"')]
    assert len(stats) == 1, r.stderr
    files = {f: md5(open(os.path.join(d, f), "rb").read()) for f in sorted(os.listdir(d)) if f not in INPUTS}
    return {"code": r.returncode, "stdout": md5(r.stdout), "stderr": md5("".join(l for l in err if l not in stats).encode()), "files": files,
            "stats_keys": list(json.loads(stats[0]))}


EXPECTED = {'profile_out_iterations': {'code': 0,
                            'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
                            'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                            'files': {'p.prof': '38ec2fe44ca35a848cfd0e2aeeb09350'},
                            'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                                           'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                                           'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'default_c1': {'code': 0,
                'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
                'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                'files': {},
                'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                               'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                               'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'default_c2': {'code': 0,
                'stdout': '3fba653d45f282b1c7297da8abf44e62',
                'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                'files': {},
                'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                               'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                               'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'i3': {'code': 0,
        'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
        'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
        'files': {},
        'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s', 'merge_profiles_s',
                       'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports', 'bionj_s',
                       'bionj_device_calls', 'bionj_launches', 'switches']},
 't': {'code': 0,
       'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
       'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
       'files': {},
       'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s', 'merge_profiles_s',
                      'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports', 'bionj_s',
                      'bionj_device_calls', 'bionj_launches', 'switches']},
 'topology': {'code': 0,
              'stdout': 'a2aeaf9a5694fa8f009cc558fcb2366f',
              'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
              'files': {},
              'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                             'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                             'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'T': {'code': 0,
       'stdout': 'a9a1326cf6569d0ba1011eb4524e256c',
       'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
       'files': {},
       'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s', 'merge_profiles_s',
                      'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports', 'bionj_s',
                      'bionj_device_calls', 'bionj_launches', 'switches']},
 'T_bootstrap_ml_tree': {'code': 0,
                         'stdout': 'a9a1326cf6569d0ba1011eb4524e256c',
                         'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                         'files': {'b.nwk': '675d8ae5311aad9af6985f0e31a0a601', 'm.nwk': 'd5033fc8471561f3f1e61e8af2e852bc'},
                         'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                                        'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                                        'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches', 'bootstrap_replicates',
                                        'bootstrap_s', 'bootstrap_counts_calls', 'ml_tree_s', 'ml_rounds', 'ml_evaluations', 'ml_lnl_start', 'ml_lnl',
                                        'ml_kernel_ms']},
 'r': {'code': 0,
       'stdout': '35b15866af61d15c89e5b0ae1110e587',
       'stderr': '117f5cf267d7184ac36a03484b810f29',
       'files': {},
       'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s', 'merge_profiles_s',
                      'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports', 'bionj_s',
                      'bionj_device_calls', 'bionj_launches', 'switches', 'reroot', 'reroot_merges', 'reroot_candidates', 'reroot_heights',
                      'reroot_batches', 'reroot_align_s', 'reroot_host_merge_s', 'reroot_gapmask_s', 'reroot_parsimony_s', 'reroot_rows_s']},
 'rr': {'code': 0,
        'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
        'stderr': '3fca2273287c716a49963d2a4f9ad9b6',
        'files': {},
        'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s', 'merge_profiles_s',
                       'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports', 'bionj_s',
                       'bionj_device_calls', 'bionj_launches', 'switches', 'reroot', 'reroot_merges', 'reroot_candidates', 'reroot_heights',
                       'reroot_batches', 'reroot_align_s', 'reroot_host_merge_s', 'reroot_gapmask_s', 'reroot_parsimony_s', 'reroot_rows_s']},
 'W': {'code': 0,
       'stdout': '8f9b91580b6c32322b38478f1aee64ff',
       'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
       'files': {},
       'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s', 'merge_profiles_s',
                      'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports', 'bionj_s',
                      'bionj_device_calls', 'bionj_launches', 'switches', 'wls_refine', 'wls_trees', 'wls_s', 'wls_pair_sums_s', 'wls_kernels_s',
                      'wls_sweeps', 'wls_quartets', 'wls_quintets', 'wls_batches', 'wls_launches']},
 'R_read_repeats': {'code': 0,
                    'stdout': '6275d028ca785a6d16f3e46a84bc0636',
                    'stderr': '155dfc0aa2289ec0928cc7e8d739c637',
                    'files': {},
                    'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                                   'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                                   'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'profile_out': {'code': 0,
                 'stdout': '64edaf76db6d6e60dc4248fe36f3607f',
                 'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                 'files': {'p.prof': 'eeccfafcd3d408e8f66e4186bc2bbe2a'},
                 'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                                'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                                'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'cs_profile': {'code': 0,
                'stdout': '112495d4bc3ece0bf98d3c1f665c5a07',
                'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                'files': {},
                'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                               'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                               'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'codon': {'code': 0,
           'stdout': 'd8181a1466d1b2af647fdaa4e47521d1',
           'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
           'files': {},
           'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                          'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports',
                          'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'ancestral_seqs': {'code': 0,
                    'stdout': '517706180ba36fc29f4c1402dd45d3a8',
                    'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                    'files': {},
                    'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                                   'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                                   'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'early_refinement': {'code': 0,
                      'stdout': 'b138fcc82105fa0d3f4b0a0029660d71',
                      'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
                      'files': {},
                      'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                                     'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                                     'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches']},
 'guidance': {'code': 0,
              'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
              'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
              'files': {'g.res': '162d91f7189c9abf89c98ee87e5e29de',
                        'g.txt': 'b213af82c425ff290f2976c72242fac9',
                        'gd.0.fa': 'a2aeaf9a5694fa8f009cc558fcb2366f',
                        'gd.0.nwk': 'e49f61ee5caa53edbe336e8998ef7028',
                        'gd.1.fa': 'c961cceaa93dcc793c042b713cc0fe66',
                        'gd.1.nwk': '7c346cc248ef2d2ea6dae193ad9a49aa',
                        'gd.2.fa': 'a2aeaf9a5694fa8f009cc558fcb2366f',
                        'gd.2.nwk': '05c4f916670a1e8898b7a510c213f6e2'},
              'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                             'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                             'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches', 'guidance_replicates', 'guidance_s',
                             'guidance_align_s', 'guidance_agreement_s', 'guidance_passes', 'guidance_agreement_calls']},
 'bootstrap': {'code': 0,
               'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
               'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
               'files': {'b.edges': '316fb7dae0e15abd1cec916dd86a08c3',
                         'b.nwk': '197080f248d842693a682a374d343c59',
                         'b.taxa': '4eef4a1fc9672ca163b58a86958931e0',
                         'b.tbe': '13d24317f9422b394075579e22e7ebb5',
                         'b.trees': 'a184bf1244c2fed1165517e7c177c786'},
               'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                              'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                              'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches', 'bootstrap_replicates',
                              'bootstrap_s', 'bootstrap_counts_calls', 'bootstrap_tbe_s', 'bootstrap_transfer_calls', 'bootstrap_transfer_kernel_ms',
                              'bootstrap_taxa_s', 'bootstrap_taxa_calls', 'bootstrap_taxa_kernel_ms']},
 'ml_gamma': {'code': 0,
              'stdout': 'c961cceaa93dcc793c042b713cc0fe66',
              'stderr': 'd41d8cd98f00b204e9800998ecf8427e',
              'files': {'m.nwk': '87cabf841d6e25f50cfbdeb14a1f46fb',
                        'm.rates': '4f8e71f709c76b227111bf711c7ddcea',
                        'm.sites': '273c48e9e6a9e5846e3d885aaf66810e'},
              'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                             'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident',
                             'resident_imports', 'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches', 'ml_tree_s', 'ml_rounds',
                             'ml_evaluations', 'ml_lnl_start', 'ml_lnl', 'ml_kernel_ms', 'ml_categories', 'ml_alpha']},
 'batch': {'code': 2,
           'stdout': 'd41d8cd98f00b204e9800998ecf8427e',
           'stderr': '4162c928f6dba680684300f61c51dfcc',
           'files': {'o1.fa': 'c961cceaa93dcc793c042b713cc0fe66', 'o3.fa': '64edaf76db6d6e60dc4248fe36f3607f'},
           'stats_keys': ['backend', 'init_s', 'tree_s', 'progressive_s', 'align_cells', 'align_s', 'nw_cells', 'nw_s', 'mldist_s',
                          'merge_profiles_s', 'farm_workers', 'farm_tiles', 'farm_level_workers', 'farm_leaf_workers', 'resident', 'resident_imports',
                          'bionj_s', 'bionj_device_calls', 'bionj_launches', 'switches', 'batch_families', 'batch_failed', 'batch_chunks',
                          'batch_passes', 'batch_levels', 'batch_align_calls', 'batch_dist_calls']}}


@pytest.fixture(scope="module")
def exe(oracle_build):
    return os.path.join(oracle_build, "pgmsa_oracle")


def test_the_table_covers_what_it_should():
    assert sorted(CASES) == sorted(EXPECTED)
    assert sum(len(e["files"]) for e in EXPECTED.values()) >= 20 and EXPECTED["batch"]["code"] == 2
    assert all(e["code"] == 0 for n, e in EXPECTED.items() if n != "batch")
    assert not any(k.startswith("batch_") for n, e in EXPECTED.items() if n != "batch" for k in e["stats_keys"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_as_the_parent_commit(exe, tmp_path, name):
    got = record(exe, name, tmp_path)
    for key in ("code", "stats_keys", "stderr", "stdout", "files"):
        assert got[key] == EXPECTED[name][key], (name, key)


def test_only_tree_with_both_analyses_writes_what_each_writes_alone(exe, tmp_path):
    """`-T --bootstrap 4 --bootstrap_out B --ml_tree M`: the final alignment both need is computed once; B and M are the files of
    `-T --bootstrap 4 --bootstrap_out B` and of `-T --ml_tree M`."""
    fa = os.path.join(GOLD, "c1.fa")
    p = lambda n: str(tmp_path / n)
    both = bu.run(exe, ["-T", "--bootstrap", "4", "--bootstrap_out", p("B2"), "--ml_tree", p("M2"), fa])
    b = bu.run(exe, ["-T", "--bootstrap", "4", "--bootstrap_out", p("B1"), fa])
    m = bu.run(exe, ["-T", "--ml_tree", p("M1"), fa])
    assert both.stdout == b.stdout == m.stdout and both.stdout.count("(") > 0
    assert open(p("B2")).read() == open(p("B1")).read() and open(p("B1")).read().count("(") > 0
    assert open(p("M2")).read() == open(p("M1")).read() and open(p("M1")).read().count("(") > 0


def test_solo_trees_come_from_the_per_family_calls(exe, tmp_path):
    """Outputs and `--stats` keys are the same whether the solo run estimates its trees through TreeNJ (the per-family backend
    calls) or through TreeNJ_multi, so neither can tell the two apart.  With PGM_HOST_PROFILE set, the TreeNJ branch of the loop
    (trees_for, host/driver_family.cpp) prints `guide tree from the alignment:` once per re-estimated tree, as the solo loop of
    8881cb7 did (its driver prints one such line for c1.fa, whose second round converges, and two for c2.fa); the TreeNJ_multi
    branch, which a `--batch` run of the same family takes, prints none."""
    env = dict(os.environ, PGM_HOST_PROFILE="1")
    lines = lambda r: [l for l in r.stderr.splitlines() if l.startswith("guide tree from the alignment: ")]
    for fa, n in (("c1.fa", 1), ("c2.fa", 2)):
        assert len(lines(bu.run(exe, ["--fasta", os.path.join(GOLD, fa)], env=env))) == n, fa
    lst = str(tmp_path / "one.list")
    bu.write_list(lst, [os.path.join(GOLD, "c1.fa")], [str(tmp_path / "o.fa")])
    assert lines(bu.run(exe, ["--fasta", "--batch", lst], env=env)) == []
    assert open(str(tmp_path / "o.fa")).read() == open(os.path.join(GOLD, "c1.default.out.fa")).read()


FA = os.path.join(GOLD, "c1.fa")
BOOT = ["--bootstrap", "4", "--bootstrap_out", "B"]
GUID = ["--guidance", "4", "--guidance_out", "G"]
BATCH = "ERROR:--batch cannot be combined with "
# (arguments, exit code, the whole of stderr; None: the usage text); the messages are those of 8881cb7's parser
REFUSALS = [
    (["--batch", "L", FA], 2, BATCH + "a positional sequence file (the families come from the list)"),
    (["--batch", "L", "-o", "x"], 2, BATCH + "-o (every line of the list names its output)"),
    (["--batch", "L", "-t", "x"], 2, BATCH + "-t (a guide tree is the third field of a family's line)"),
    (["--batch", "L", "--topology", "x"], 2, BATCH + "--topology (a topology is the fourth field of a family's line)"),
    (["--batch", "L", "-r"], 2, BATCH + "-r"),
    (["--batch", "L", "--reroot"], 2, BATCH + "-r"),
    (["--batch", "L", "-W"], 2, BATCH + "-W"),
    (["--batch", "L", "--wls_refine"], 2, BATCH + "-W"),
    (["--batch", "L", "-R"], 2, BATCH + "-R"),
    (["--batch", "L", "--read_repeats", "x"], 2, BATCH + "--read_repeats"),
    (["--batch", "L", "--profile_out", "x"], 2, BATCH + "--profile_out"),
    (["--batch", "L", "--dump_jobs", "x"], 2, BATCH + "--dump_jobs"),
    (["--batch", "L", "--dump_dist", "x"], 2, BATCH + "--dump_dist"),
    (["--batch", "L", "--dump_joins", "x"], 2, BATCH + "--dump_joins"),
    (["--batch", "L"] + BOOT, 2, BATCH + "--bootstrap"),
    (["--batch", "L", "--bootstrap_seed", "3", "--bootstrap_tbe", "x"], 2, BATCH + "--bootstrap"),
    (["--batch", "L"] + GUID, 2, BATCH + "--guidance"),
    (["--batch", "L", "--guidance_residues", "x"], 2, BATCH + "--guidance"),
    (["--batch", "L", "--guidance_dump", "x"], 2, BATCH + "--guidance"),
    (["--batch", "L", "--ml_tree", "x"], 2, BATCH + "--ml_tree"),
    (["--batch", "L", "-r", "-W", "-o", "x"], 2, BATCH + "-o (every line of the list names its output)"),   # (the first arm that holds)
    (["--dna", "--codon", FA], 2, "ERROR:--dna cannot be combined with --codon"),
    (["--dna", "-c", "x", FA], 2, "ERROR:--dna cannot be combined with -c (context-specific profiles are amino-acid profiles)"),
    (["--dna", "--codon", "-c", "x", FA], 2, "ERROR:--dna cannot be combined with --codon"),
    (["-r", "--ancestral_seqs", FA], 2, "ERROR:--ancestral_seqs and --profile_out cannot be combined with -r (the root search keeps no ancestral profiles)"),
    (["-rr", "--profile_out", "x", FA], 2, "ERROR:--ancestral_seqs and --profile_out cannot be combined with -r (the root search keeps no ancestral profiles)"),
    (["--no_such_flag", FA], 1, "Command line error: unknown flag --no_such_flag"),
    ([FA, "-Wr"], 1, "Command line error: unknown flag -Wr"),
    ([FA, "-t"], 1, None),
    (["--bootstrap_out"], 1, None),
    ([], 1, None),
    (["--fasta", "-T"], 1, None),
    # the numbers: the whole text must be one, and within the bounds
    (BOOT + ["--bootstrap", "0", FA], 2, "ERROR:--bootstrap takes a number of replicates from 1 to 1000"),
    (BOOT + ["--bootstrap", "1001", FA], 2, "ERROR:--bootstrap takes a number of replicates from 1 to 1000"),
    (GUID + ["--guidance", "0", FA], 2, "ERROR:--guidance takes a number of replicates from 1 to 1000"),
    (GUID + ["--guidance", "1001", FA], 2, "ERROR:--guidance takes a number of replicates from 1 to 1000"),
    (["--guidance_dump", "x", FA], 2, "ERROR:--guidance_residues and --guidance_dump need --guidance"),
] + [
    (BOOT + ["--bootstrap_taxa", "x", "--bootstrap_taxa_cutoff", v, FA], 2, "ERROR:--bootstrap_taxa_cutoff takes a number X with 0 <= X < 1")
    for v in ("", "x", "0.3x", "1", "-0.1", "nan")
] + [
    (["--ml_tree", "M", "--ml_rounds", v, FA], 2, "ERROR:--ml_rounds takes a number of rounds from 1 to 10000") for v in ("", "5x", "2.5", "0", "10001")
] + [
    (["--ml_tree", "M", "--ml_epsilon", v, FA], 2, "ERROR:--ml_epsilon takes a number X >= 0") for v in ("", "1e-3x", "-1", "inf", "nan")
] + [
    (["--ml_tree", "M", "--ml_gamma", v, FA], 2, "ERROR:--ml_gamma takes a number of categories from 2 to 16") for v in ("", "4x", "1", "17")
] + [
    (["--ml_tree", "M", "--ml_gamma", "4", "--ml_alpha", v, FA], 2, "ERROR:--ml_alpha takes a number X with 0.05 <= X <= 100") for v in ("", "1x", "0.04", "101", "nan")
] + [
    # a command line that is wrong twice gets the message of the refusal tested first
    (["--ml_tree", "M", "--ml_gamma", "1", "--ml_alpha", "0", "--ml_rounds", "0", "--ml_epsilon", "-1", "-W", FA], 2, "ERROR:--ml_gamma takes a number of categories from 2 to 16"),
    (["--ml_tree", "M", "--ml_gamma", "4", "--ml_alpha", "0", "--ml_rounds", "0", "--ml_epsilon", "-1", "-W", FA], 2, "ERROR:--ml_alpha takes a number X with 0.05 <= X <= 100"),
    (["--ml_tree", "M", "--ml_rounds", "0", "--ml_epsilon", "-1", "-W", FA], 2, "ERROR:--ml_rounds takes a number of rounds from 1 to 10000"),
    (["--ml_tree", "M", "--ml_epsilon", "-1", "-W", FA], 2, "ERROR:--ml_epsilon takes a number X >= 0"),
    (["--ml_rounds", "0", "--ml_gamma", "1", FA], 2, "ERROR:--ml_sites, --ml_rounds and --ml_epsilon need --ml_tree"),
    (BOOT + ["--bootstrap", "0", "--bootstrap_taxa_cutoff", "2", "-W", FA], 2, "ERROR:--bootstrap takes a number of replicates from 1 to 1000"),
    (BOOT + ["--bootstrap_taxa_cutoff", "2", "-W", FA], 2, "ERROR:--bootstrap_taxa_cutoff and --bootstrap_taxa_edges need --bootstrap_taxa"),
    (BOOT + ["--bootstrap_taxa", "x", "--bootstrap_taxa_cutoff", "2", "-W", FA], 2, "ERROR:--bootstrap_taxa_cutoff takes a number X with 0 <= X < 1"),
    (BOOT + GUID + ["--ml_tree", "M", "-W", "-r", FA], 2, "ERROR:--bootstrap cannot be combined with -W"),
    (GUID + ["--ml_tree", "M", "-T", "-W", FA], 2, "ERROR:--guidance cannot be combined with -T (there is no alignment to score)"),
    (["--batch", "L", "--dna", "--codon"] + BOOT, 2, BATCH + "--bootstrap"),
    (BOOT + ["--dna", "--codon", "-r", "--ancestral_seqs", FA], 2, "ERROR:--bootstrap cannot be combined with -r"),
    (["--dna", "--codon", "-r", "--ancestral_seqs", FA], 2, "ERROR:--ancestral_seqs and --profile_out cannot be combined with -r (the root search keeps no ancestral profiles)"),
]


@pytest.fixture(scope="module")
def usage_text(exe):
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "" and r.stderr.startswith("USAGE: pgmsa ") and md5(r.stderr.encode()) == USAGE_MD5
    return r.stderr


USAGE_MD5 = "a2dc25cc791db6206d56ef535b7380f4"


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusals(exe, usage_text, tmp_path, k):
    args, code, msg = REFUSALS[k]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == code and r.stdout == "", (args, r.returncode, r.stderr)
    assert r.stderr == (usage_text if msg is None else msg + "\n"), args
    assert os.listdir(str(tmp_path)) == []   # (refused before anything is opened)


def test_oracle_rebuilds_after_an_included_file_changes(tmp_path):
    """`make -C oracle` in a copy of the tree: up to date after a build, out of date once treelik_internal.h (included by
    treelik.cpp) is touched, up to date again after the next build."""
    root = str(tmp_path / "tree")
    for d in ("oracle", "include", os.path.join("prographmsa_amd", "host"), os.path.join("prographmsa_amd", "csrc")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(root, d), ignore=shutil.ignore_patterns("_build", "_ref", "*.so", "*.o", "data"))
    old = os.stat(root).st_mtime - 1000
    for base, _, files in os.walk(root):
        for f in files:
            os.utime(os.path.join(base, f), (old, old))
    # (the dependencies do not depend on the optimisation level: -O0 keeps the two builds short)
    make = lambda *a: subprocess.run(["make", "-s", "-C", os.path.join(root, "oracle"), "CXXFLAGS=-O0 -std=c++17 -ffp-contract=off -pthread"] + list(a),
                                     capture_output=True, text=True, timeout=600)
    first = make()
    assert first.returncode == 0, first.stderr
    assert make("-q").returncode == 0
    build = os.path.join(root, "oracle", "_build")
    for f in os.listdir(build):   # (the products older than the touch below, newer than every source)
        os.utime(os.path.join(build, f), (old + 500, old + 500))
    assert make("-q").returncode == 0
    os.utime(os.path.join(root, "prographmsa_amd", "host", "treelik_internal.h"))
    assert make("-q").returncode == 1
    again = make()
    assert again.returncode == 0, again.stderr
    assert make("-q").returncode == 0
