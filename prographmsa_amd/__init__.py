"""prographmsa_amd — MI355X (gfx950) accelerator for ProGraphMSA's graph-vs-graph DP hot path.

The product is the C-ABI shared library ``lib/libpgm_hip.so`` (HIP kernels, see ``include/pgm_hip.h``)
plus the C++ host mirror of the reference call surface (``host/``, driver ``bin/pgmsa``).  This Python
package is plumbing only: a ctypes binding of the C ABI for the tests and ``bench.py``.

There is no CPU fallback: importing works without a GPU (symbols can be inspected), but every compute
entry point needs a gfx950 device, and a missing library raises ``ImportError`` at import time.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpgm_hip.so")
PGMSA_PATH = os.path.join(_HERE, "bin", "pgmsa")

PGM_OK, PGM_ERR_INVALID, PGM_ERR_DEVICE, PGM_ERR_BACKTRACK, PGM_ERR_NOMEM = 0, 1, 2, 3, 4
PGM_GAP = 0xFFFFFFFF
PGM_BATCH_KEEP_MATRICES = 1
PGM_NW_REDUCED = 1
PGM_MERGE_RESIDENT = 1


class pgm_graph(C.Structure):
    _fields_ = [("n", C.c_uint32), ("dim", C.c_uint32), ("sites", C.POINTER(C.c_double)),
                ("e_rowptr", C.POINTER(C.c_int32)), ("e_col", C.POINTER(C.c_uint32)), ("e_val", C.POINTER(C.c_float)),
                ("r_rowptr", C.POINTER(C.c_int32)), ("r_col", C.POINTER(C.c_uint32)), ("r_units", C.POINTER(C.c_uint32))]


class pgm_model(C.Structure):
    _fields_ = [("M", C.POINTER(C.c_double)), ("pi", C.POINTER(C.c_double))]


class pgm_scores(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("gap_init", "gap_extend", "match_init", "end_match", "end_gap", "end_skip",
                                         "start_gap", "start_init", "repeat_init", "repeat_ext")]


class pgm_mldist_model(C.Structure):
    _fields_ = [("dim", C.c_uint32), ("Q", C.POINTER(C.c_double)), ("V", C.POINTER(C.c_double)), ("Vi", C.POINTER(C.c_double)),
                ("sigma", C.POINTER(C.c_double))] + [(n, C.c_double) for n in ("dist_max", "var_max", "var_min", "cutoff_dist", "min_dist", "max_dist", "indel_rate")] \
        + [("mldist", C.c_int32), ("mldist_gap", C.c_int32)]


class pgm_merge_job(C.Structure):
    _fields_ = [("dim", C.c_uint32), ("n1", C.c_uint32), ("n2", C.c_uint32), ("nnodes", C.c_uint32),
                ("sites1", C.POINTER(C.c_double)), ("sites2", C.POINTER(C.c_double)), ("P1", C.POINTER(C.c_double)), ("P2", C.POINTER(C.c_double)),
                ("k1", C.POINTER(C.c_uint32)), ("k2", C.POINTER(C.c_uint32)), ("g2_with_P1", C.POINTER(C.c_uint8)), ("profiles", C.POINTER(C.c_double))]


class pgm_site_ref(C.Structure):
    _fields_ = [("dev_sites", C.POINTER(C.c_double)), ("node_map", C.POINTER(C.c_uint32)), ("ncols", C.c_uint32)]


class pgm_gapmask_job(C.Structure):
    _fields_ = [("src", C.POINTER(C.c_uint64)), ("mapping", C.POINTER(C.c_uint32)), ("dst", C.POINTER(C.c_uint64)),
                ("nrows", C.c_uint32), ("ncols_in", C.c_uint32), ("ncols_out", C.c_uint32)]


class pgm_parsimony_job(C.Structure):
    _fields_ = [("masks", C.POINTER(C.c_uint64)), ("children", C.POINTER(C.c_uint32)), ("nleaves", C.c_uint32), ("ncols", C.c_uint32)]


class pgm_wls_job(C.Structure):
    _fields_ = [("label", C.POINTER(C.c_int8)), ("offset", C.POINTER(C.c_double)), ("nsub", C.c_uint32)]


class pgm_bionj_join(C.Structure):
    _fields_ = [("index1", C.c_uint32), ("index2", C.c_uint32), ("dist1", C.c_double), ("dist2", C.c_double)]


class pgm_bionj_pair(C.Structure):
    _fields_ = [("index1", C.c_uint32), ("index2", C.c_uint32)]


class pgm_align_out(C.Structure):
    _fields_ = [("score", C.c_float), ("n_tr_indels", C.c_uint32), ("len", C.c_uint32), ("status", C.c_int32),
                ("map1", C.POINTER(C.c_uint32)), ("map2", C.POINTER(C.c_uint32))]


# every symbol include/pgm_hip.h declares
EXPORTS = [
    "pgm_device_count", "pgm_ctx_create", "pgm_ctx_destroy", "pgm_last_error", "pgm_ctx_device_info",
    "pgm_align_graphs_batch", "pgm_align_batch_create", "pgm_align_batch_create_ex", "pgm_align_batch_create_res", "pgm_align_graphs_batch_res", "pgm_align_batch_run", "pgm_align_batch_fetch",
    "pgm_align_batch_destroy", "pgm_align_batch_cells", "pgm_align_batch_test_stall", "pgm_test_cu_shares", "pgm_test_batch_plan", "pgm_align_batch_stage_times", "pgm_align_batch_job_times", "pgm_align_batch_time", "pgm_align_batch_read_matrices",
    "pgm_nw_pairs_batch", "pgm_nw_pairs_submit", "pgm_nw_pairs_wait", "pgm_nw_last_kernel_ms", "pgm_host_alloc", "pgm_host_free", "pgm_csprofile_load", "pgm_csprofile_create_batch", "pgm_csprofile_create_batch_res",
    "pgm_csprofile_last_kernel_ms", "pgm_mldist_batch", "pgm_prealigned_counts_batch", "pgm_kmer_cosine", "pgm_dist_last_kernel_ms",
    "pgm_kmer_cosine_multi", "pgm_prealigned_counts_multi", "pgm_prealigned_counts_resampled",
    "pgm_merge_profiles_batch", "pgm_merge_profiles_batch_ex", "pgm_resident_reset", "pgm_resident_onehot", "pgm_resident_import", "pgm_merge_last_kernel_ms",
    "pgm_gapmask_extend_batch", "pgm_gap_parsimony_batch", "pgm_parsimony_last_kernel_ms",
    "pgm_wls_load", "pgm_wls_pair_sums_batch", "pgm_wls_last_kernel_ms", "pgm_wls_last_launches",
    "pgm_bionj", "pgm_bionj_multi", "pgm_bionj_last_launches", "pgm_bionj_last_kernel_ms",
    "pgm_bionj_plan", "pgm_bionj_plan_multi",
    "pgm_msa_agreement", "pgm_agreement_last_kernel_ms",
    "pgm_transfer_min", "pgm_transfer_last_kernel_ms", "pgm_transfer_taxa",
    "pgm_tree_likelihood", "pgm_treelik_last_kernel_ms", "pgm_tree_likelihood_rates", "pgm_tree_ancestral", "pgm_tree_nni", "pgm_tree_nni_edge", "pgm_tree_spr",
    "pgm_tree_ancestral_joint", "pgm_tree_ancestral_sample",
    "pgm_resampled_sums", "pgm_resample_last_kernel_ms",
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libpgm_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "— there is no CPU fallback for the hot path" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    PG, PM = C.POINTER(C.POINTER(pgm_graph)), C.POINTER(C.POINTER(pgm_model))
    sig = {
        "pgm_device_count": (C.c_int, []),
        "pgm_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "pgm_ctx_destroy": (None, [vp]),
        "pgm_last_error": (C.c_char_p, []),
        "pgm_ctx_device_info": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
        "pgm_align_graphs_batch": (C.c_int, [vp, u32, PG, PG, PM, C.POINTER(pgm_scores), C.POINTER(pgm_align_out)]),
        "pgm_align_batch_create": (C.c_int, [vp, u32, PG, PG, PM, C.POINTER(pgm_scores), C.POINTER(vp)]),
        "pgm_align_batch_create_ex": (C.c_int, [vp, u32, PG, PG, PM, C.POINTER(pgm_scores), u32, C.POINTER(vp)]),
        "pgm_align_batch_create_res": (C.c_int, [vp, u32, PG, PG, PM, C.POINTER(pgm_scores), u32, C.POINTER(pgm_site_ref), C.POINTER(pgm_site_ref), C.POINTER(vp)]),
        "pgm_align_graphs_batch_res": (C.c_int, [vp, u32, PG, PG, PM, C.POINTER(pgm_scores), C.POINTER(pgm_site_ref), C.POINTER(pgm_site_ref), C.POINTER(pgm_align_out)]),
        "pgm_align_batch_run": (C.c_int, [vp, vp]),
        "pgm_align_batch_fetch": (C.c_int, [vp, vp, C.POINTER(pgm_align_out)]),
        "pgm_align_batch_destroy": (None, [vp, vp]),
        "pgm_align_batch_cells": (C.c_uint64, [vp]),
        "pgm_align_batch_test_stall": (C.c_int, [vp, u32, u32, u32]),
        "pgm_test_cu_shares": (C.c_int, [u32, C.c_double, u32, C.c_double, u32, C.c_double, u32, u32, C.c_double, C.POINTER(C.c_uint32)]),
        "pgm_test_batch_plan": (C.c_int, [u32, PG, PG, PM, C.POINTER(pgm_scores), u32, C.POINTER(pgm_site_ref), C.POINTER(pgm_site_ref), u32,
                                          C.POINTER(u32), C.POINTER(C.c_double)] + [C.POINTER(u32)] * 4 + [C.POINTER(i32)]),
        "pgm_align_batch_stage_times": (C.c_int, [vp, C.c_int] + [C.POINTER(C.c_float)] * 3 + [C.POINTER(u32)]),
        "pgm_align_batch_job_times": (C.c_int, [vp, vp, C.POINTER(C.c_uint64)]),
        "pgm_align_batch_time": (C.c_int, [vp, vp, C.c_int] + [C.POINTER(C.c_float)] * 4),
        "pgm_align_batch_read_matrices": (C.c_int, [vp, vp, u32] + [C.POINTER(C.c_float)] * 5),
        "pgm_nw_pairs_batch": (C.c_int, [vp, u32, C.POINTER(i32), i32, i32, u32, C.POINTER(C.c_int8), C.POINTER(u32), u32,
                                         C.POINTER(u32), C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]),
        "pgm_nw_pairs_submit": (C.c_int, [vp, u32, C.POINTER(i32), i32, i32, u32, C.POINTER(C.c_int8), C.POINTER(u32), u32,
                                          C.POINTER(u32), C.POINTER(u32), u32, C.POINTER(i32), C.POINTER(u32), C.POINTER(C.c_int)]),
        "pgm_nw_pairs_wait": (C.c_int, [vp, C.c_int]),
        "pgm_host_alloc": (vp, [C.c_size_t]),
        "pgm_host_free": (None, [vp]),
        "pgm_nw_last_kernel_ms": (C.c_float, [vp]),
        "pgm_csprofile_load": (C.c_int, [vp, u32, u32] + [C.POINTER(C.c_double)] * 3),
        "pgm_csprofile_create_batch": (C.c_int, [vp, u32, C.POINTER(C.c_int8), C.POINTER(u32)] + [C.POINTER(C.c_double)] * 4
                                       + [C.POINTER(C.c_uint64)]),
        "pgm_csprofile_create_batch_res": (C.c_int, [vp, u32, C.POINTER(C.c_int8), C.POINTER(u32)] + [C.POINTER(C.c_double)] * 3
                                           + [C.POINTER(C.POINTER(C.c_double))]),
        "pgm_csprofile_last_kernel_ms": (C.c_float, [vp]),
        "pgm_mldist_batch": (C.c_int, [vp, C.POINTER(pgm_mldist_model), u32, C.POINTER(i32), C.POINTER(u32)] + [C.POINTER(C.c_double)] * 3),
        "pgm_prealigned_counts_batch": (C.c_int, [vp, u32, u32, u32, C.POINTER(C.c_int8), u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]),
        "pgm_kmer_cosine": (C.c_int, [vp, u32, u32, C.POINTER(i32), C.POINTER(C.c_double)]),
        "pgm_dist_last_kernel_ms": (C.c_float, [vp]),
        "pgm_kmer_cosine_multi": (C.c_int, [vp, u32, C.POINTER(u32), u32, C.POINTER(i32), C.POINTER(C.c_double)]),
        "pgm_prealigned_counts_multi": (C.c_int, [vp, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_int8), u32, C.POINTER(u32), C.POINTER(u32),
                                                  C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]),
        "pgm_prealigned_counts_resampled": (C.c_int, [vp, u32, u32, u32, C.POINTER(C.c_int8), u32, C.POINTER(u32), u32, C.POINTER(u32), C.POINTER(u32),
                                                      C.POINTER(i32), C.POINTER(u32)]),
        "pgm_merge_profiles_batch": (C.c_int, [vp, u32, C.POINTER(pgm_merge_job)]),
        "pgm_merge_profiles_batch_ex": (C.c_int, [vp, u32, C.POINTER(pgm_merge_job), u32, C.POINTER(C.POINTER(C.c_double))]),
        "pgm_resident_reset": (C.c_int, [vp]),
        "pgm_resident_onehot": (C.c_int, [vp, u32, u32, C.POINTER(C.c_int8), C.POINTER(u32), C.POINTER(C.POINTER(C.c_double))]),
        "pgm_resident_import": (C.c_int, [vp, vp, C.POINTER(C.c_double), C.c_uint64, C.POINTER(C.POINTER(C.c_double))]),
        "pgm_merge_last_kernel_ms": (C.c_float, [vp]),
        "pgm_gapmask_extend_batch": (C.c_int, [vp, u32, C.POINTER(pgm_gapmask_job)]),
        "pgm_gap_parsimony_batch": (C.c_int, [vp, u32, C.POINTER(pgm_parsimony_job), C.POINTER(u32)]),
        "pgm_parsimony_last_kernel_ms": (C.c_float, [vp]),
        "pgm_wls_load": (C.c_int, [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "pgm_wls_pair_sums_batch": (C.c_int, [vp, u32, C.POINTER(pgm_wls_job), C.POINTER(C.c_double)]),
        "pgm_wls_last_kernel_ms": (C.c_float, [vp]),
        "pgm_wls_last_launches": (C.c_uint32, [vp]),
        "pgm_bionj": (C.c_int, [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(pgm_bionj_join), C.POINTER(C.c_double)]),
        "pgm_bionj_multi": (C.c_int, [vp, u32, C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(pgm_bionj_join), C.POINTER(C.c_double)]),
        "pgm_bionj_last_launches": (C.c_uint32, [vp]),
        "pgm_bionj_last_kernel_ms": (C.c_float, [vp]),
        "pgm_bionj_plan": (C.c_int, [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(pgm_bionj_pair), C.POINTER(pgm_bionj_join), C.POINTER(C.c_double)]),
        "pgm_bionj_plan_multi": (C.c_int, [vp, u32, C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(pgm_bionj_pair), C.POINTER(pgm_bionj_join), C.POINTER(C.c_double)]),
        "pgm_msa_agreement": (C.c_int, [vp, u32, u32, u32, C.POINTER(i32), C.POINTER(u32), C.POINTER(u32)]),
        "pgm_agreement_last_kernel_ms": (C.c_float, [vp]),
        "pgm_transfer_min": (C.c_int, [vp, u32, u32, C.POINTER(C.c_uint64), u32, C.POINTER(u32), C.POINTER(C.c_uint64), C.POINTER(u32)]),
        "pgm_transfer_last_kernel_ms": (C.c_float, [vp]),
        "pgm_transfer_taxa": (C.c_int, [vp, u32, u32, C.POINTER(C.c_uint64), C.POINTER(u32), u32, C.POINTER(u32), C.POINTER(C.c_uint64),
                                        C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "pgm_tree_likelihood": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "pgm_treelik_last_kernel_ms": (C.c_float, [vp]),
        "pgm_tree_likelihood_rates": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                                C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.POINTER(C.c_double)]),
        "pgm_tree_ancestral": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_int8),
                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "pgm_tree_nni": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(i32),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "pgm_tree_nni_edge": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "pgm_tree_spr": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(i32),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "pgm_tree_ancestral_joint": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_uint8),
                                               C.POINTER(C.c_int8), C.POINTER(C.c_double), C.POINTER(i32)]),
        "pgm_tree_ancestral_sample": (C.c_int, [vp, u32, u32, u32, C.POINTER(u32), u32, C.POINTER(C.c_int8), C.POINTER(C.c_double), u32, C.POINTER(C.c_double),
                                                C.POINTER(C.c_double), u32, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_double),
                                                C.POINTER(C.c_uint8), C.POINTER(C.c_int8)]),
        "pgm_resampled_sums": (C.c_int, [vp, u32, u32, C.POINTER(C.c_double), u32, C.POINTER(u32), C.POINTER(C.c_double)]),
        "pgm_resample_last_kernel_ms": (C.c_float, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError here = the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class PgmError(RuntimeError):
    pass


def check(rc, what="libpgm_hip"):
    if rc != PGM_OK:
        raise PgmError("%s failed (%d): %s" % (what, rc, lib.pgm_last_error().decode()))


class Context:
    """pgm_ctx wrapper.  Raises PgmError when no gfx950 device is usable (no CPU fallback)."""

    def __init__(self, device=0):
        self.handle = C.c_void_p()
        check(lib.pgm_ctx_create(device, C.byref(self.handle)), "pgm_ctx_create")

    def device_info(self):
        buf = C.create_string_buffer(256)
        cu = C.c_int()
        check(lib.pgm_ctx_device_info(self.handle, buf, 256, C.byref(cu)))
        return buf.value.decode(), cu.value

    def prealigned_counts_resampled(self, dim, rows, cols, pi, pj):
        """pgm_prealigned_counts_resampled: rows (nrows x ncols int8), cols (nrep x ncols source columns), the pairs (pi, pj) ->
        counts (nrep x npairs x dim * dim int32) and gaps (nrep x npairs uint32)."""
        import numpy as np
        rows = np.ascontiguousarray(rows, np.int8)
        cols = np.ascontiguousarray(cols, np.uint32)
        pi = np.ascontiguousarray(pi, np.uint32)
        pj = np.ascontiguousarray(pj, np.uint32)
        nrep, npairs = cols.shape[0], len(pi)
        counts = np.zeros((nrep, npairs, dim * dim), np.int32)
        gaps = np.zeros((nrep, npairs), np.uint32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_prealigned_counts_resampled(self.handle, dim, rows.shape[0], rows.shape[1], P(rows, C.c_int8), nrep, P(cols, C.c_uint32), npairs,
                                                  P(pi, C.c_uint32), P(pj, C.c_uint32), P(counts, C.c_int32), P(gaps, C.c_uint32)), "pgm_prealigned_counts_resampled")
        return counts, gaps

    def msa_agreement(self, where, res_hits=None, pair_hits=None):
        """pgm_msa_agreement: where (nrep x nrows x ncols int32, negative = gap) -> res_hits (nrows x ncols uint32) and pair_hits
        (nrows x nrows uint32).  Given output arrays (C-contiguous uint32 of those shapes) are overwritten in place."""
        import numpy as np
        where = np.ascontiguousarray(where, np.int32)
        nrep, nrows, ncols = where.shape
        if res_hits is None: res_hits = np.zeros((nrows, ncols), np.uint32)
        if pair_hits is None: pair_hits = np.zeros((nrows, nrows), np.uint32)
        for o, shape in ((res_hits, (nrows, ncols)), (pair_hits, (nrows, nrows))):
            if o.dtype != np.uint32 or o.shape != shape or not o.flags.c_contiguous: raise ValueError("msa_agreement: output array of the wrong kind")
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_msa_agreement(self.handle, nrows, ncols, nrep, P(where, C.c_int32), P(res_hits, C.c_uint32), P(pair_hits, C.c_uint32)), "pgm_msa_agreement")
        return res_hits, pair_hits

    def transfer_min(self, nleaves, ref, rep_off, rep, phi=None):
        """pgm_transfer_min: ref (nref x words uint64, words = (nleaves + 63) // 64), rep_off (nrep + 1 uint32), rep (rep_off[-1] x words
        uint64) -> phi (nref x nrep uint32).  A given output array (C-contiguous uint32 of that shape) is overwritten in place."""
        import numpy as np
        words = (nleaves + 63) // 64
        ref = np.ascontiguousarray(ref, np.uint64)
        rep_off = np.ascontiguousarray(rep_off, np.uint32)
        rep = np.ascontiguousarray(rep, np.uint64).reshape(-1, words)
        if ref.ndim != 2 or ref.shape[1] != words or rep_off.ndim != 1 or len(rep_off) < 1 or rep.shape[0] != int(rep_off[-1]):
            raise ValueError("transfer_min: input array of the wrong shape")
        nref, nrep = ref.shape[0], len(rep_off) - 1
        if phi is None: phi = np.zeros((nref, nrep), np.uint32)
        if phi.dtype != np.uint32 or phi.shape != (nref, nrep) or not phi.flags.c_contiguous: raise ValueError("transfer_min: output array of the wrong kind")
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_transfer_min(self.handle, nleaves, nref, P(ref, C.c_uint64), nrep, P(rep_off, C.c_uint32), P(rep, C.c_uint64) if rep.size else None,
                                   P(phi, C.c_uint32)), "pgm_transfer_min")
        return phi

    def transfer_taxa(self, nleaves, ref, thr, rep_off, rep, out=None):
        """pgm_transfer_taxa: inputs as transfer_min plus thr (nref uint32) -> (phi, arg (nref x nrep), moved (nref x nleaves),
        counted (nref)), all uint32.  Given output arrays (a tuple of four, C-contiguous uint32 of those shapes) are overwritten."""
        import numpy as np
        words = (nleaves + 63) // 64
        ref = np.ascontiguousarray(ref, np.uint64)
        thr = np.ascontiguousarray(thr, np.uint32)
        rep_off = np.ascontiguousarray(rep_off, np.uint32)
        rep = np.ascontiguousarray(rep, np.uint64).reshape(-1, words)
        if ref.ndim != 2 or ref.shape[1] != words or thr.shape != (ref.shape[0],) or rep_off.ndim != 1 or len(rep_off) < 1 or rep.shape[0] != int(rep_off[-1]):
            raise ValueError("transfer_taxa: input array of the wrong shape")
        nref, nrep = ref.shape[0], len(rep_off) - 1
        shapes = [(nref, nrep), (nref, nrep), (nref, nleaves), (nref,)]
        if out is None: out = tuple(np.zeros(s, np.uint32) for s in shapes)
        if len(out) != 4 or any(a.dtype != np.uint32 or a.shape != s or not a.flags.c_contiguous for a, s in zip(out, shapes)):
            raise ValueError("transfer_taxa: output array of the wrong kind")
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_transfer_taxa(self.handle, nleaves, nref, P(ref, C.c_uint64), P(thr, C.c_uint32), nrep, P(rep_off, C.c_uint32),
                                    P(rep, C.c_uint64) if rep.size else None, *[P(a, C.c_uint32) for a in out]), "pgm_transfer_taxa")
        return tuple(out)

    def tree_likelihood(self, dim, parent, rows, pi, P, derivs=True, out=None):
        """pgm_tree_likelihood: parent (nnodes uint32, the root's 0xffffffff), rows (nleaves x ncols int8), pi (dim), P ((nnodes - 1) x
        {3 with derivs, else 1} x dim x dim float64, every matrix column-major) -> (site_l (ncols float64), site_k (ncols int32),
        d1, d2 (nnodes - 1 float64; left as given without derivs)).  Given output arrays (a tuple of four, C-contiguous of those
        kinds) are overwritten."""
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        if parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or P.size != (len(parent) - 1) * (3 if derivs else 1) * dim * dim:
            raise ValueError("tree_likelihood: input array of the wrong shape")
        nnodes, (nleaves, ncols) = len(parent), rows.shape
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((nnodes - 1,), np.float64), ((nnodes - 1,), np.float64)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 4 or any(a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_likelihood: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_likelihood(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), P_(P, C.c_double),
                                      1 if derivs else 0, P_(out[0], C.c_double), P_(out[1], C.c_int32), P_(out[2], C.c_double), P_(out[3], C.c_double)),
              "pgm_tree_likelihood")
        return tuple(out)

    def tree_likelihood_rates(self, dim, parent, rows, pi, w, P, derivs=True, out=None):
        """pgm_tree_likelihood_rates: as tree_likelihood with the weights w (ncat) and P (ncat x (nnodes - 1) x {3 with derivs, else 1} x
        dim x dim float64, category-major) -> (site_l, site_k, post (ncat x ncols float64), d1, d2).  Given output arrays (a tuple
        of five, C-contiguous of those kinds) are overwritten; d1 and d2 are left as given without derivs."""
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        if parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or w.ndim != 1 or P.size != len(w) * (len(parent) - 1) * (3 if derivs else 1) * dim * dim:
            raise ValueError("tree_likelihood_rates: input array of the wrong shape")
        nnodes, (nleaves, ncols), ncat = len(parent), rows.shape, len(w)
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((nnodes - 1,), np.float64), ((nnodes - 1,), np.float64)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 5 or any(a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_likelihood_rates: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_likelihood_rates(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat,
                                            P_(w, C.c_double), P_(P, C.c_double), 1 if derivs else 0, P_(out[0], C.c_double), P_(out[1], C.c_int32),
                                            P_(out[2], C.c_double), P_(out[3], C.c_double), P_(out[4], C.c_double)), "pgm_tree_likelihood_rates")
        return tuple(out)

    def tree_ancestral(self, dim, parent, rows, pi, w, P, full=True, out=None):
        """pgm_tree_ancestral: inputs as tree_likelihood_rates without derivs (P: ncat x (nnodes - 1) x dim x dim float64) -> (site_l,
        site_k, post, anc_state (ninner x ncols int8), anc_prob (ninner x ncols float64), anc_post (ninner x ncols x dim float64)),
        ninner = nnodes - nleaves.  Given output arrays (a tuple of six, C-contiguous of those kinds) are overwritten; without `full`
        the entry gets no anc_post: a given one is left as it is (it may be None), and None is returned in its place otherwise."""
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        if parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or w.ndim != 1 or P.size != len(w) * (len(parent) - 1) * dim * dim or len(parent) <= rows.shape[0]:
            raise ValueError("tree_ancestral: input array of the wrong shape")
        nnodes, (nleaves, ncols), ncat = len(parent), rows.shape, len(w)
        ninner = nnodes - nleaves
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((ninner, ncols), np.int8), ((ninner, ncols), np.float64),
                 ((ninner, ncols, dim), np.float64)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds[:5]) + ((np.zeros(*kinds[5]) if full else None),)
        right = lambda a, kind: isinstance(a, np.ndarray) and a.dtype == kind[1] and a.shape == kind[0] and a.flags.c_contiguous
        if len(out) != 6 or not all(right(a, kind) for a, kind in zip(out[:5], kinds)) or not (right(out[5], kinds[5]) or (out[5] is None and not full)):
            raise ValueError("tree_ancestral: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_ancestral(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat,
                                     P_(w, C.c_double), P_(P, C.c_double), P_(out[0], C.c_double), P_(out[1], C.c_int32), P_(out[2], C.c_double),
                                     P_(out[3], C.c_int8), P_(out[4], C.c_double), P_(out[5], C.c_double) if full else None), "pgm_tree_ancestral")
        return tuple(out)

    def _tree_ancestral_inputs(self, what, dim, parent, rows, pi, w, P):
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        if parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or w.ndim != 1 or P.size != len(w) * (len(parent) - 1) * dim * dim or len(parent) <= rows.shape[0]:
            raise ValueError("%s: input array of the wrong shape" % what)
        return parent, rows, pi, w, P

    def tree_ancestral_joint(self, dim, parent, rows, pi, w, P, out=None):
        """pgm_tree_ancestral_joint: inputs as tree_ancestral -> (site_l, site_k, post, cat (ncols uint8), joint_state (ninner x ncols
        int8), joint_l (ncols float64), joint_k (ncols int32)).  Given output arrays (a tuple of seven, C-contiguous of those kinds)
        are overwritten."""
        import numpy as np
        parent, rows, pi, w, P = self._tree_ancestral_inputs("tree_ancestral_joint", dim, parent, rows, pi, w, P)
        nnodes, (nleaves, ncols), ncat = len(parent), rows.shape, len(w)
        ninner = nnodes - nleaves
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((ncols,), np.uint8), ((ninner, ncols), np.int8), ((ncols,), np.float64),
                 ((ncols,), np.int32)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 7 or any(not isinstance(a, np.ndarray) or a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_ancestral_joint: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_ancestral_joint(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat,
                                           P_(w, C.c_double), P_(P, C.c_double), P_(out[0], C.c_double), P_(out[1], C.c_int32), P_(out[2], C.c_double),
                                           P_(out[3], C.c_uint8), P_(out[4], C.c_int8), P_(out[5], C.c_double), P_(out[6], C.c_int32)), "pgm_tree_ancestral_joint")
        return tuple(out)

    def tree_ancestral_sample(self, dim, parent, rows, pi, w, P, nsamp, seed, first_sample=0, out=None):
        """pgm_tree_ancestral_sample: inputs as tree_ancestral; the samples first_sample .. first_sample + nsamp - 1 of the stream of
        `seed` -> (site_l, site_k, post, samp_cat (ncols x nsamp uint8), samp_state (ninner x ncols x nsamp int8)).  Given output arrays
        (a tuple of five, C-contiguous of those kinds) are overwritten."""
        import numpy as np
        parent, rows, pi, w, P = self._tree_ancestral_inputs("tree_ancestral_sample", dim, parent, rows, pi, w, P)
        nsamp, seed, first_sample = int(nsamp), int(seed), int(first_sample)
        if not (0 < nsamp < 2 ** 32 and 0 <= seed < 2 ** 64 and 0 <= first_sample < 2 ** 64):
            raise ValueError("tree_ancestral_sample: nsamp, seed or first_sample out of range")
        nnodes, (nleaves, ncols), ncat = len(parent), rows.shape, len(w)
        ninner = nnodes - nleaves
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((ncols, nsamp), np.uint8), ((ninner, ncols, nsamp), np.int8)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 5 or any(not isinstance(a, np.ndarray) or a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_ancestral_sample: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_ancestral_sample(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat,
                                            P_(w, C.c_double), P_(P, C.c_double), nsamp, first_sample, seed, P_(out[0], C.c_double), P_(out[1], C.c_int32),
                                            P_(out[2], C.c_double), P_(out[3], C.c_uint8), P_(out[4], C.c_int8)), "pgm_tree_ancestral_sample")
        return tuple(out)

    def tree_nni(self, dim, parent, rows, pi, w, P, cand, out=None):
        """pgm_tree_nni: inputs as tree_ancestral; cand: ncand x 3 uint32, a row (v, a, c) -> (site_l, site_k, post, rho (ncand x ncols
        float64)).  Given output arrays (a tuple of four, C-contiguous of those kinds) are overwritten."""
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        cand = np.asarray(cand, np.uint32)
        if parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or w.ndim != 1 or P.size != len(w) * (len(parent) - 1) * dim * dim or cand.ndim != 2 or cand.shape[1] != 3:
            raise ValueError("tree_nni: input array of the wrong shape")
        nnodes, (nleaves, ncols), ncat, ncand = len(parent), rows.shape, len(w), len(cand)
        cv, ca, cc = (np.ascontiguousarray(cand[:, k]) for k in range(3))
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((ncand, ncols), np.float64)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 4 or any(a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_nni: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_nni(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat, P_(w, C.c_double),
                               P_(P, C.c_double), ncand, P_(cv, C.c_uint32), P_(ca, C.c_uint32), P_(cc, C.c_uint32), P_(out[0], C.c_double), P_(out[1], C.c_int32),
                               P_(out[2], C.c_double), P_(out[3], C.c_double)), "pgm_tree_nni")
        return tuple(out)

    def tree_nni_edge(self, dim, parent, rows, pi, w, P, cand, Pc, out=None):
        """pgm_tree_nni_edge: inputs as tree_nni; Pc: ncat x ncand x 3 x dim x dim float64, the candidates' own P, P', P'' of the edge
        above v -> (site_l, site_k, post, rho (ncand x ncols float64), d1, d2 (ncand float64)).  Given output arrays (a tuple of six,
        C-contiguous of those kinds) are overwritten."""
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        Pc = np.ascontiguousarray(Pc, np.float64)
        cand = np.asarray(cand, np.uint32)
        if (parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or w.ndim != 1 or P.size != len(w) * (len(parent) - 1) * dim * dim or cand.ndim != 2
                or cand.shape[1] != 3 or Pc.size != len(w) * len(cand) * 3 * dim * dim):
            raise ValueError("tree_nni_edge: input array of the wrong shape")
        nnodes, (nleaves, ncols), ncat, ncand = len(parent), rows.shape, len(w), len(cand)
        cv, ca, cc = (np.ascontiguousarray(cand[:, k]) for k in range(3))
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((ncand, ncols), np.float64), ((ncand,), np.float64), ((ncand,), np.float64)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 6 or any(a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_nni_edge: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_nni_edge(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat, P_(w, C.c_double),
                                    P_(P, C.c_double), ncand, P_(cv, C.c_uint32), P_(ca, C.c_uint32), P_(cc, C.c_uint32), P_(Pc, C.c_double), P_(out[0], C.c_double),
                                    P_(out[1], C.c_int32), P_(out[2], C.c_double), P_(out[3], C.c_double), P_(out[4], C.c_double), P_(out[5], C.c_double)),
              "pgm_tree_nni_edge")
        return tuple(out)

    def tree_spr(self, dim, parent, rows, pi, w, P, Ph, cand, out=None):
        """pgm_tree_spr: inputs as tree_nni; Ph: the shape of P, the matrix of half of every edge; cand: ncand x 2 uint32, a row (v, y)
        -> (site_l, site_k, post, rho (ncand x ncols float64)).  Given output arrays (a tuple of four, C-contiguous of those kinds) are
        overwritten."""
        import numpy as np
        parent = np.ascontiguousarray(parent, np.uint32)
        rows = np.ascontiguousarray(rows, np.int8)
        pi = np.ascontiguousarray(pi, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        Ph = np.ascontiguousarray(Ph, np.float64)
        cand = np.asarray(cand, np.uint32)
        if (parent.ndim != 1 or rows.ndim != 2 or pi.shape != (dim,) or w.ndim != 1 or P.size != len(w) * (len(parent) - 1) * dim * dim or Ph.size != P.size
                or cand.ndim != 2 or cand.shape[1] != 2):
            raise ValueError("tree_spr: input array of the wrong shape")
        nnodes, (nleaves, ncols), ncat, ncand = len(parent), rows.shape, len(w), len(cand)
        cv, cy = (np.ascontiguousarray(cand[:, k]) for k in range(2))
        kinds = [((ncols,), np.float64), ((ncols,), np.int32), ((ncat, ncols), np.float64), ((ncand, ncols), np.float64)]
        if out is None: out = tuple(np.zeros(s, t) for s, t in kinds)
        if len(out) != 4 or any(a.dtype != t or a.shape != s or not a.flags.c_contiguous for a, (s, t) in zip(out, kinds)):
            raise ValueError("tree_spr: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_tree_spr(self.handle, dim, nleaves, nnodes, P_(parent, C.c_uint32), ncols, P_(rows, C.c_int8), P_(pi, C.c_double), ncat, P_(w, C.c_double),
                               P_(P, C.c_double), P_(Ph, C.c_double), ncand, P_(cv, C.c_uint32), P_(cy, C.c_uint32), P_(out[0], C.c_double), P_(out[1], C.c_int32),
                               P_(out[2], C.c_double), P_(out[3], C.c_double)), "pgm_tree_spr")
        return tuple(out)

    def resampled_sums(self, x, cols, out=None):
        """pgm_resampled_sums: x nrow x ncols float64 (no NaN, no +inf), cols nrep x ncols uint32 -> out (nrow x nrep float64),
        out[q, r] = the sum over k ascending of x[q, cols[r, k]].  A given output array (C-contiguous of that kind) is overwritten."""
        import numpy as np
        x = np.ascontiguousarray(x, np.float64)
        cols = np.ascontiguousarray(cols, np.uint32)
        if x.ndim != 2 or cols.ndim != 2 or cols.shape[1] != x.shape[1]:
            raise ValueError("resampled_sums: input array of the wrong shape")
        (nrow, ncols), nrep = x.shape, cols.shape[0]
        if out is None: out = np.zeros((nrow, nrep), np.float64)
        if out.dtype != np.float64 or out.shape != (nrow, nrep) or not out.flags.c_contiguous:
            raise ValueError("resampled_sums: output array of the wrong kind")
        P_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        check(lib.pgm_resampled_sums(self.handle, nrow, ncols, P_(x, C.c_double), nrep, P_(cols, C.c_uint32), P_(out, C.c_double)), "pgm_resampled_sums")
        return out

    def close(self):
        if self.handle:
            lib.pgm_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
