/*
 * pgm_hip.h — C ABI of the MI355X (gfx950) accelerator for ProGraphMSA's hot path.
 *
 * The reference (acg-team/ProGraphMSA) has no plugin/FFI layer; its seams are three C++
 * functions.  Each entry point below replaces one of them (reference file:line cited per
 * function).  Plain C types only: pointers + sizes, caller-allocated outputs, `int`
 * status return (0 = PGM_OK).  The library is libpgm_hip.so (prographmsa_amd/csrc).
 *
 * The identical structs are consumed by the test-only CPU oracle (oracle/pgm_oracle.c),
 * which exports the same functions under the `pgmo_` prefix.
 */
#ifndef PGM_HIP_H_
#define PGM_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------ */
#define PGM_OK 0
#define PGM_ERR_INVALID 1    /* bad argument (null pointer, n < 2, dim mismatch ...)        */
#define PGM_ERR_DEVICE 2     /* HIP runtime error; see pgm_last_error()                     */
#define PGM_ERR_BACKTRACK 3  /* reference: error("backtracking failed") GraphAlign.h:410    */
#define PGM_ERR_NOMEM 4

#define PGM_GAP 0xFFFFFFFFu  /* (index_t)-1 in the reference's mappings                     */

/* ---- flattened reference types ------------------------------------------------------- */

/* Graph<ALPHABET> (reference src/Graph.h:31-33).  `sites` is the Eigen profile matrix
 * (dim x n, column-major, double; columns 0 and n-1 are the zero START/END columns).
 * `e_*` is the row-major CSR of `edges(to,from)`: row = node, col = predecessor (ascending),
 * value = min(cost,1e4f)-1e4f exactly as stored by Graph::setEdgesFromMap (Graph.h:85).
 * `r_*` is the CSR of `repeats(to,from)` (value = repeat-unit count); r_rowptr may be NULL
 * when the graph has no tandem-repeat edges.  Iteration order of PredIterator (Graph.h:196):
 * all e_ entries of the row, then all r_ entries. */
typedef struct pgm_graph {
    uint32_t n;
    uint32_t dim;
    const double *sites;
    const int32_t *e_rowptr; /* n+1 */
    const uint32_t *e_col;
    const float *e_val;
    const int32_t *r_rowptr; /* n+1 or NULL */
    const uint32_t *r_col;
    const uint32_t *r_units;
} pgm_graph;

/* The members of Model<ALPHABET> (reference src/Model.h:8-24) that reach alignGraphs:
 * M = diag(pi)*P(d), dim x dim column-major double; pi, dim doubles. */
typedef struct pgm_model {
    const double *M;
    const double *pi;
} pgm_model;

/* DynProgScores<ALPHABET> (reference src/GraphAlign.h:133-142), computed by the host caller
 * (it needs averageAlignmentLength and cmdlineopts) and passed by value. */
typedef struct pgm_scores {
    float gap_init, gap_extend, match_init, end_match, end_gap, end_skip;
    float start_gap, start_init, repeat_init, repeat_ext;
} pgm_scores;

/* AlignmentResult<ALPHABET> (reference src/GraphAlign.h:6-12).  map1/map2 are caller
 * allocated with capacity n1+n2 (the reference reserves the same, GraphAlign.h:297-298);
 * `len` entries are valid, PGM_GAP marks a gap, entry 0 is (0,0), the last (n1-1,n2-1). */
typedef struct pgm_align_out {
    float score;
    uint32_t n_tr_indels;
    uint32_t len;
    int32_t status; /* PGM_OK or PGM_ERR_BACKTRACK for this job */
    uint32_t *map1;
    uint32_t *map2;
} pgm_align_out;

typedef struct pgm_ctx pgm_ctx;
typedef struct pgm_align_batch pgm_align_batch;

/* ---- context ------------------------------------------------------------------------ */
int pgm_device_count(void);
/* One context per device (streams, buffer cache, resident arena).  Creation is where the start-up costs are paid: the device code
 * is loaded (an empty launch), the copy path is warmed (1 MB each way), the library's host threads are started, and the context's
 * buffer cache is filled with a first set of blocks — 128 MB + 8 MB of pinned staging memory and 3.4 GB of device memory (what the
 * levels of a 256 x 1000 or a 1024 x 600 progressive pass need; a batch that needs more replaces a block).  PGM_NO_STAGING_RESERVE=1 /
 * PGM_NO_DEVICE_RESERVE=1 in the environment: no such blocks, every batch allocates what it needs when it is created. */
int pgm_ctx_create(int device, pgm_ctx **out);
void pgm_ctx_destroy(pgm_ctx *ctx);
const char *pgm_last_error(void);
/* name of the device ("gfx950...") and CU count, for logs */
int pgm_ctx_device_info(pgm_ctx *ctx, char *name, size_t name_len, int *cu_count);

/* ---- (B1) alignGraphs  — replaces reference src/GraphAlign.h:200-534 ------------------
 * One call = njobs independent alignGraphs(g1[i], g2[i], model[i]) evaluations (the
 * reference calls it once per internal guide-tree node, ProgressiveAlignment.h:439, and
 * once per child in early refinement, :170).  Emission scores + ls_log (GraphAlign.h:146-163,
 * ls_log.h:22-59), border init (:205-234), fill (:238-260), end node (:264-280) and the
 * traceback incl. markAlternativePath (:166-198, :285-521) all run on the GPU. */
int pgm_align_graphs_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1,
                           const pgm_graph *const *g2, const pgm_model *const *model,
                           const pgm_scores *scores, pgm_align_out *out);

/* Staged form of the same call (what pgm_align_graphs_batch does internally):
 *   create  : flatten + upload every job's inputs to HBM, allocate the DP storage
 *   run     : launch the prep, emission and fill(+traceback) kernels on the context's stream (asynchronous)
 *   fetch   : wait for the stream, then copy score / mappings from the batch's pinned result block (written by the kernel
 *             itself while it runs) into caller memory
 * bench.py times `run` with the inputs already resident.
 * A stage sizes its persistent grids for the WHOLE device: between `run` and the end of `fetch` no other batch may run on that
 * device (pgm_align_graphs_batch serialises the contexts of one device itself; callers of the staged form do it themselves). */
int pgm_align_batch_create(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1,
                           const pgm_graph *const *g2, const pgm_model *const *model,
                           const pgm_scores *scores, pgm_align_batch **out);
/* The same with flags.  PGM_BATCH_KEEP_MATRICES: every job's M, X, Y, W matrices are written to device memory so that
 * pgm_align_batch_read_matrices can return them (test hook).  Without it a job of two plain chains (sequence graph against
 * sequence graph) keeps one decision byte per cell instead of the 16 bytes of the four floats: its traceback walks the
 * decisions the fill took with the operands in registers (same tie rules, GraphAlign.h:382-411), the mappings are the same.
 * If, in addition, every profile column of both graphs is one-hot, uniform (1 / dim) or empty — the leaf level of a guide tree —
 * the emission scores (GraphAlign.h:146-163) are not stored either: S(y, x) depends on the classes of row y and column x alone,
 * a (dim + 2)^2 table per job (same operations on the same operands as for any other cell: bit-identical scores). */
#define PGM_BATCH_KEEP_MATRICES 1u
int pgm_align_batch_create_ex(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1,
                              const pgm_graph *const *g2, const pgm_model *const *model,
                              const pgm_scores *scores, uint32_t flags, pgm_align_batch **out);
/* Graphs whose node profiles already are in HBM (left there by pgm_merge_profiles_batch_ex with PGM_MERGE_RESIDENT): for job i,
 * res1[i].dev_sites != NULL replaces g1[i]->sites (which may then be NULL) by that device matrix, gathered through
 * res1[i].node_map — node v of the graph handed over (a CleanedGraph, src/CleanedGraph.h:39-146) has the profile in column
 * node_map[v] of the matrix (the merged graph it was cleaned from); node_map == NULL: column v.  res1 / res2 may be NULL. */
typedef struct pgm_site_ref {
    const double *dev_sites;
    const uint32_t *node_map; /* host array, n entries */
    uint32_t ncols;           /* columns of the device matrix: every node_map[v] (or n itself, without a map) must stay below it — PGM_ERR_INVALID otherwise */
} pgm_site_ref;
int pgm_align_batch_create_res(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1,
                               const pgm_graph *const *g2, const pgm_model *const *model,
                               const pgm_scores *scores, uint32_t flags, const pgm_site_ref *res1,
                               const pgm_site_ref *res2, pgm_align_batch **out);
int pgm_align_graphs_batch_res(pgm_ctx *ctx, uint32_t njobs, const pgm_graph *const *g1,
                               const pgm_graph *const *g2, const pgm_model *const *model,
                               const pgm_scores *scores, const pgm_site_ref *res1,
                               const pgm_site_ref *res2, pgm_align_out *out);
int pgm_align_batch_run(pgm_ctx *ctx, pgm_align_batch *b);
int pgm_align_batch_fetch(pgm_ctx *ctx, pgm_align_batch *b, pgm_align_out *out);
void pgm_align_batch_destroy(pgm_ctx *ctx, pgm_align_batch *b);
/* Σ (n1-2)(n2-2) over the jobs of the batch (the GCUPS numerator). */
uint64_t pgm_align_batch_cells(const pgm_align_batch *b);
/* Run the batch `reps` times back to back and return the mean device time in milliseconds of
 * each kernel stage (prep, emission scores, fill), measured with HIP events on the context's
 * stream.  The tracebacks run inside the fill kernel (the worker that completes a job's last
 * band walks that job's path), so ms_fill includes them and ms_traceback is ~0. */
int pgm_align_batch_time(pgm_ctx *ctx, pgm_align_batch *b, int reps, float *ms_prep,
                         float *ms_emission, float *ms_fill, float *ms_traceback);
/* Mean device time (ms, HIP events on the library's stream) of the three stages — prep, emission scores, fill incl. the lean
 * jobs' kernel and all tracebacks — over the launches of pgm_align_batch_run that pgm_align_batch_fetch has completed since the
 * last reset, and their number: the stage times of exactly the steps a caller timed (bench.py), not of extra launches. */
int pgm_align_batch_stage_times(pgm_align_batch *b, int reset, float *ms_prep, float *ms_emission, float *ms_fill,
                                uint32_t *launches);
/* Timeline of the last completed launch: ticks[2 i] = the moment job i's last band was complete, ticks[2 i + 1] = the moment
 * its traceback was published, both in 10 ns ticks of the device's real-time counter (differences are meaningful, the origin
 * is not).  Tells which job's chain of sweeps, or which traceback, a batch waits for (tools/probe_jobtimes.py). */
int pgm_align_batch_job_times(pgm_ctx *ctx, pgm_align_batch *b, uint64_t *ticks);
/* Test hook for the hand-off time-out path: in the following launches band `band` of job `job` never publishes its progress
 * and a wavefront that waits for another gives up after `spin_limit` polls (0: the default); the band below then times out,
 * raises the batch's abort flag and every unfinished job reports PGM_ERR_DEVICE.  job = 0xFFFFFFFF switches it off. */
int pgm_align_batch_test_stall(pgm_align_batch *b, uint32_t job, uint32_t band, uint32_t spin_limit);
/* Test hook (host arithmetic only, no device call): how `cus` compute units are dealt to the launches of a batch's fill stage —
 * out4 = {lean queue, band queue, launch of the longest chains, main launch} — given each queue's work in microseconds of one
 * worker, its number of units (lean jobs, bands, items of the main launch, items of the longest chains) and the longest chain
 * of sweeps in microseconds.  Every queue with work gets at least one CU and the shares never exceed `cus`. */
int pgm_test_cu_shares(uint32_t cus, double lean_cost, uint32_t nlean, double band_cost, uint32_t nbands, double rest_cost,
                       uint32_t nrest, uint32_t ncrit, double longest_chain, uint32_t *out4);
/* Test hook (host arithmetic only, no device call): the plan pgm_align_batch_create_res makes for these jobs on a device of `cus`
 * compute units, through the same functions (csrc/pgm_plan.h), in caller memory.  Invalid input: the codes and messages of create.
 *   head   PGM_PLAN_HEAD words: dp of the jobs (0: no job), promote_bands, nitems, ncrit, nbands, nbands_narrow, nlean, ntb, ntb_c, ntb_b,
 *          the workers nworkers, nlean, nband, nwide, ncrit, ntb, ntb_b, then crit_c3, rest_c3 and of the PGM_HOST_PROFILE "work lists:"
 *          line the main launch's CUs, the narrow bands, the main launch's items, the items of the longest chains
 *   dhead  PGM_PLAN_DHEAD doubles, the rest of that line: longest chain of sweeps, goal, lean cost, band cost, simulated end of the bands,
 *          cost and simulated end of the items, simulated end of the longest chains; then longest_crit_chain
 *   job_fields  PGM_PLAN_JOB words per job: lean, has_extras, mode2, hD, hDX, slot_bytes, aux_off, ov_off, rh_off, c3_off, nov2, has_far,
 *          long1, long2, crit3, far_slack, nslots, generic nodes, kill nodes
 *   items, bands  {job, band, prio, count} per entry, room for one entry per band of 64 rows of the batch;  lean_list  njobs words;
 *   tblist  {job, last item} per entry, njobs entries */
#define PGM_PLAN_HEAD 23
#define PGM_PLAN_DHEAD 9
#define PGM_PLAN_JOB 19
int pgm_test_batch_plan(uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2, const pgm_model *const *model,
                        const pgm_scores *scores, uint32_t flags, const pgm_site_ref *res1, const pgm_site_ref *res2, uint32_t cus,
                        uint32_t *head, double *dhead, uint32_t *job_fields, uint32_t *items, uint32_t *bands, uint32_t *lean_list, int32_t *tblist);
/* Test hook: copy one job's DP matrices back as the reference lays them out (n1 x n2,
 * column-major, element (y,x) at y + x*n1).  Only rows < n1-1 and columns < n2-1 are
 * defined (the END row/column are never written by the reference's fill either).
 * Any of M,X,Y,W may be NULL.  S is the emission matrix of GraphAlign.h:146-163 (PGM_ERR_INVALID for a job of two sequence graphs
 * in a batch without PGM_BATCH_KEEP_MATRICES: its scores were never stored). */
int pgm_align_batch_read_matrices(pgm_ctx *ctx, pgm_align_batch *b, uint32_t job, float *M,
                                  float *X, float *Y, float *W, float *S);

/* ---- (B2) DistanceFactoryAlign::alignPair — replaces reference
 * src/DistanceFactoryAlign.h:59-127 (called from computePwDistances, :29-56).
 * syms: concatenated sequences already mapped through ALPHABET::value() with negative
 * values replaced by 20 (the reference's quirk, :72,79); offs[nseq+1] delimits them.
 * score: (dim+1)x(dim+1) int32 column-major scoring matrix (DistanceFactoryAlign.cpp).
 * For pair p = (pi[p], pj[p]) with seq1 = sequence pi, seq2 = sequence pj the call returns
 * counts[p*dim*dim + s1 + dim*s2] (the reference's CountMatrix counts(s1,s2), column-major)
 * and gaps[p] (number of gap openings on the traceback path). */
int pgm_nw_pairs_batch(pgm_ctx *ctx, uint32_t dim, const int32_t *score, int32_t gap_open,
                       int32_t gap_extend, uint32_t nseq, const int8_t *syms,
                       const uint32_t *offs, uint32_t npairs, const uint32_t *pi,
                       const uint32_t *pj, int32_t *counts, uint32_t *gaps);
/* The same in two halves, so that a caller keeps TWO tiles of pairs in flight on one context: submit returns once the tile's
 * inputs are staged and its kernel and copies are enqueued (ticket 0 or 1); wait blocks until that tile's results are in
 * `counts` / `gaps` (the pointers given to submit, which must stay valid until then).  While the host waits for tile k and
 * copies its count matrices out, the kernel of tile k+1 runs.  A third submit without a wait is refused (PGM_ERR_INVALID).
 * flags: PGM_NW_REDUCED — `counts` receives two int32 per pair, (Σ_s counts(s,s), Σ counts), instead of the dim x dim matrix:
 * all the p-distance of DistanceFactoryML.h:143-146 reads (the default flow without --mldist).
 * Result buffers from pgm_host_alloc (pinned) are written by the D2H copy directly; any other memory goes through the
 * library's pinned staging block and one host copy.  One host thread per context. */
#define PGM_NW_REDUCED 1u
int pgm_nw_pairs_submit(pgm_ctx *ctx, uint32_t dim, const int32_t *score, int32_t gap_open,
                        int32_t gap_extend, uint32_t nseq, const int8_t *syms,
                        const uint32_t *offs, uint32_t npairs, const uint32_t *pi,
                        const uint32_t *pj, uint32_t flags, int32_t *counts, uint32_t *gaps, int *ticket);
int pgm_nw_pairs_wait(pgm_ctx *ctx, int ticket);
/* Device-time of the NW kernel of the tile the last pgm_nw_pairs_wait / pgm_nw_pairs_batch on this context completed (ms;
 * with two tiles in flight the second kernel's blocks wait for the first's to leave, so the times of overlapping tiles
 * overlap too). */
float pgm_nw_last_kernel_ms(pgm_ctx *ctx);
/* Pinned host memory for result buffers (NULL on failure). */
void *pgm_host_alloc(size_t bytes);
void pgm_host_free(void *p);

/* ---- (B3) CSProfile::createProfile — replaces reference src/CSProfile.cpp:175-225 ------
 * load: K context profiles with `ncols` window columns.  lprofiles: K x ncols x 21 doubles
 * (weights already applied, last entry of each row = 0, CSProfile.cpp:157-162), row-major
 * [k][col][symbol]; centre: K x 20 doubles = profiles_k.row(center); priors: K doubles
 * (= log(PRIOR)).  create: for each sequence (symbols 0..19, 20 = invalid) writes the
 * 20 x (L+2) column-major double profile of Model<AA>::Profile into out + out_offs[s].
 * tau[s] = model.divergence/0.8; pi = model.pi (20); p_uniform = model.P * (1/20), one vector of
 * 20 per sequence (nseq x 20, each leaf has its own model). */
int pgm_csprofile_load(pgm_ctx *ctx, uint32_t K, uint32_t ncols, const double *lprofiles,
                       const double *centre, const double *priors);
int pgm_csprofile_create_batch(pgm_ctx *ctx, uint32_t nseq, const int8_t *syms,
                               const uint32_t *offs, const double *tau, const double *pi,
                               const double *p_uniform, double *out, const uint64_t *out_offs);
/* The same with the profiles left in HBM (the leaf graphs of a resident pass, as pgm_resident_onehot for plain sequence graphs):
 * dev[s] = the 20 x (L_s + 2) matrix of sequence s in the context's resident arena (valid until pgm_resident_reset), to be named by
 * pgm_site_ref / pgm_merge_job; nothing is copied back. */
int pgm_csprofile_create_batch_res(pgm_ctx *ctx, uint32_t nseq, const int8_t *syms,
                                   const uint32_t *offs, const double *tau, const double *pi,
                                   const double *p_uniform, const double **dev);
float pgm_csprofile_last_kernel_ms(pgm_ctx *ctx);

/* ---- (f3) DistanceFactoryML::computeDistance / computeMLDist — replaces reference
 * src/DistanceFactoryML.h:66-190 for a batch of pairs (the tail of computePwDistances, src/DistanceFactoryAlign.h:49-51,
 * and of DistanceFactoryPrealigned, src/DistanceFactoryPrealigned.h:84-88).  The substitution model is handed over in the
 * eigen form the reference builds in ModelFactory (src/ModelFactory.h:48-67): P(d) = V diag(exp(sigma d)) V^-1, all
 * dim x dim matrices column-major double; dim <= 20: the kernel keeps P(d) and its two derivatives of one pair in the registers
 * of one wavefront (20 x 20 / 64 lanes).  Or in the general form: Q alone, V == Vi == sigma == NULL, dim <= 64 (the 61-state
 * codon model, any generator without a usable eigen form): P(d) = exp(Q d) by scaling and squaring with 20 Taylor terms, the
 * steps and the order of host/model_factory.cpp's expm, one workgroup per pair.  PGM_ERR_INVALID: an eigen form with
 * dim > 20, a general form with dim > 64, only some of V, Vi, sigma given.  min_dist / max_dist are the clamps of parseDistance
 * (src/ModelFactory.h:125), dist_max / var_max / var_min the constants of DistanceFactoryML.cpp:3-32.
 * counts[p * dim * dim + s1 + dim * s2], gaps[p], seqlen[p] = (L1 + L2) / 2 per pair -> dist[p], var[p]. */
typedef struct pgm_mldist_model {
    uint32_t dim;
    const double *Q, *V, *Vi, *sigma;   /* general form: V == Vi == sigma == NULL */
    double dist_max, var_max, var_min, cutoff_dist, min_dist, max_dist, indel_rate;
    int32_t mldist, mldist_gap; /* cmdlineopts.mldist_flag / mldist_gap_flag */
} pgm_mldist_model;
int pgm_mldist_batch(pgm_ctx *ctx, const pgm_mldist_model *model, uint32_t npairs, const int32_t *counts,
                     const uint32_t *gaps, const double *seqlen, double *dist, double *var);

/* ---- (f3) DistanceFactoryPrealigned pair counts — replaces the column loop of reference
 * src/DistanceFactoryPrealigned.h:34-90.  rows: nrows x ncols int8, row-major: ALPHABET::value() of a residue
 * (0..dim-1), -1 for a gap, -2 for a residue without a value.  Only values < 20 are counted (the reference's literal 20).
 * counts[p * dim * dim + s1 + dim * s2] and gaps[p] (gap openings) per pair (pi[p], pj[p]). */
int pgm_prealigned_counts_batch(pgm_ctx *ctx, uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows,
                                uint32_t npairs, const uint32_t *pi, const uint32_t *pj, int32_t *counts,
                                uint32_t *gaps);
/* ---- (f4) DistanceFactoryAngle's cosine matrix — replaces the dense product of reference src/DistanceFactoryAngle.h:100
 * (`norms^-1 * counts2^T * counts2 * norms^-1`, the default initial distances without -a).  counts: nseq x ncols int32,
 * row-major (row i = the K-mer counts of sequence i; ncols = DIM^K).  cosine: nseq x nseq doubles, column-major,
 * cosine(i, j) = (sum_k (c_ik / |c_i|) c_jk) / |c_j| with k ascending (fp64, one multiply and one add per term), summed in the
 * depth blocks of the reference's GEMM — L1d / 128 terms each, L1d = 49152 bytes unless the environment names the size the
 * reference's host reports (PGM_EIGEN_L1D).  The matrix is NOT symmetric in its last bits; element (i, j) is at i + nseq j. */
int pgm_kmer_cosine(pgm_ctx *ctx, uint32_t nseq, uint32_t ncols, const int32_t *counts, double *cosine);
/* ---- (f3, f4) for many families in one launch (pgmsa --batch).
 * pgm_kmer_cosine_multi: counts holds the families' count rows back to back (sum of nseq[f] rows of ncols int32), cosine their
 * nseq[f] x nseq[f] column-major matrices back to back; every element has the bits pgm_kmer_cosine gives the family alone.
 * pgm_prealigned_counts_multi: rows holds every family's nrows[f] x ncols[f] int8 matrix back to back; pair p compares rows pi[p],
 * pj[p] of family fam[p]; counts and gaps are laid out as pgm_prealigned_counts_batch lays them out (1 <= dim <= 64; a result
 * matrix smaller than 20 x 20 keeps that corner of the counts).  PGM_ERR_INVALID: a null pointer, nfam == 0, a family with fewer
 * than 2 rows, fam[p] >= nfam, a pair index outside its family. */
int pgm_kmer_cosine_multi(pgm_ctx *ctx, uint32_t nfam, const uint32_t *nseq, uint32_t ncols, const int32_t *counts, double *cosine);
int pgm_prealigned_counts_multi(pgm_ctx *ctx, uint32_t dim, uint32_t nfam, const uint32_t *nrows, const uint32_t *ncols,
                                const int8_t *rows, uint32_t npairs, const uint32_t *fam, const uint32_t *pi, const uint32_t *pj,
                                int32_t *counts, uint32_t *gaps);
/* ---- (f3) for nrep resamplings of the columns of one alignment in one launch (pgmsa --bootstrap).  Replicate r is the alignment
 * whose column k is column cols[r * ncols + k] of rows; counts[(r * npairs + p) * dim * dim + s1 + dim * s2] and gaps[r * npairs + p]
 * are what pgm_prealigned_counts_batch gives pair p on that gathered matrix (its gap openings are the gathered matrix's), the rows
 * uploaded once (1 <= dim <= 64; a result matrix smaller than 20 x 20 keeps that corner of the counts).  PGM_ERR_INVALID, before
 * anything is launched: a null pointer, nrep == 0, nrows < 2, ncols == 0, dim outside 1..64, a pair index >= nrows, a cols entry
 * >= ncols. */
int pgm_prealigned_counts_resampled(pgm_ctx *ctx, uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t nrep,
                                    const uint32_t *cols, uint32_t npairs, const uint32_t *pi, const uint32_t *pj, int32_t *counts,
                                    uint32_t *gaps);
/* Device time of the kernel of the last pgm_mldist_batch / pgm_prealigned_counts_* / pgm_kmer_cosine call on this context (ms). */
float pgm_dist_last_kernel_ms(pgm_ctx *ctx);

/* ---- (f1, numeric part) mergeGraphs' node profiles — replaces the P*g products and the L2 normalisation of reference
 * src/GraphAlign.h:569-620 for a batch of merges (one per internal guide-tree node of a level,
 * src/ProgressiveAlignment.h:449).  The caller walks the two mappings (the "unify" loops) and lists, per node of the
 * merged graph, the source node in g1 / g2 (PGM_GAP if none) and whether the g2 node is propagated with model1.P (the
 * reference does that for skipped g2 nodes, :591); the device returns the dim x nnodes profile matrix, bit-identical to
 * the reference's arithmetic (Eigen gemv association, sequential norm, multiplication by the reciprocal).  The edge lists
 * of the merged graph stay with the caller (host maps, O(edges)). */
typedef struct pgm_merge_job {
    uint32_t dim, n1, n2, nnodes;
    const double *sites1, *sites2; /* Graph::sites of the two (uncleaned) graphs, dim x n column-major */
    const double *P1, *P2;         /* model1.P, model2.P, dim x dim column-major */
    const uint32_t *k1, *k2;       /* nnodes each */
    const uint8_t *g2_with_P1;     /* nnodes */
    double *profiles;              /* out: dim x nnodes column-major */
} pgm_merge_job;
int pgm_merge_profiles_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_merge_job *jobs);
/* The same with the results LEFT IN HBM (flags & PGM_MERGE_RESIDENT): dev_profiles[i] receives the device address of job i's
 * dim x nnodes matrix, jobs[i].profiles may be NULL and nothing is copied back; sites1 / sites2 of a job may themselves be such
 * addresses (the children's profiles never left the device).  The matrices stay valid until pgm_resident_reset(ctx), which
 * a caller issues at the start of a progressive pass (the memory is kept and handed out again); they are read by the
 * alignments (pgm_site_ref) and merges of the levels above. */
#define PGM_MERGE_RESIDENT 1u
int pgm_merge_profiles_batch_ex(pgm_ctx *ctx, uint32_t njobs, const pgm_merge_job *jobs, uint32_t flags,
                                const double **dev_profiles);
int pgm_resident_reset(pgm_ctx *ctx);
/* The leaf graphs of a pass built in HBM — replaces the profile matrix of reference src/SequenceGraph.h:101-109 for nseq
 * sequences: syms = ALPHABET::value() per residue, negative for a residue without a value (uniform 1 / dim column); dev[s]
 * receives the device address of sequence s's dim x (L + 2) matrix (START and END columns zero), valid until
 * pgm_resident_reset.  Used through pgm_site_ref and as sites1 / sites2 of pgm_merge_profiles_batch_ex. */
int pgm_resident_onehot(pgm_ctx *ctx, uint32_t dim, uint32_t nseq, const int8_t *syms, const uint32_t *offs,
                        const double **dev);
/* A resident matrix of another context copied into this one's resident memory (a pass sharded over several devices by subtree: the
 * parent of two subtrees needs both children's profiles on its device; hipMemcpyPeer between devices, a device-to-device copy within
 * one).  src must be an address pgm_merge_profiles_batch_ex / pgm_resident_onehot / pgm_resident_import returned for src_ctx and
 * still be valid there; *dst stays valid until pgm_resident_reset(ctx). */
int pgm_resident_import(pgm_ctx *ctx, pgm_ctx *src_ctx, const double *src, uint64_t count, const double **dst);
float pgm_merge_last_kernel_ms(pgm_ctx *ctx);

/* ---- root search: gap masks and gap parsimony (reference src/FindRoot.h, src/GapParsimony.h) ----------------------- */
/* A gap mask holds one bit per column per row, set where the row has a gap: row r is words [r * W, (r + 1) * W) with
 * W = ceil(ncols / 64), column c is bit c % 64 of word c / 64; bits past ncols are ignored on input and zero on output. */

/* extend_alignment (reference src/ProgressiveAlignment.h:245-264) in bit form: the nrows rows of src (ncols_in columns) as rows
 * of a merged alignment of ncols_out columns.  mapping[j] (j < ncols_out) is the node of the child's graph behind merged column
 * j, PGM_GAP for none: a mapped column takes the child's next column in rank order, an unmapped one is a gap.  The non-gap
 * entries of mapping must number exactly ncols_in (PGM_ERR_INVALID otherwise).  All jobs of a call run in one launch. */
typedef struct pgm_gapmask_job {
    const uint64_t *src;       /* nrows x ceil(ncols_in / 64) words */
    const uint32_t *mapping;   /* ncols_out entries */
    uint64_t *dst;             /* out: nrows x ceil(ncols_out / 64) words */
    uint32_t nrows, ncols_in, ncols_out;
} pgm_gapmask_job;
int pgm_gapmask_extend_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_gapmask_job *jobs);

/* GapParsimony::scoreAlignment (reference src/GapParsimony.h:100-125) of many candidate alignments in one launch: Fitch
 * parsimony of the residue / gap pattern, columns in blocks of 32 as the reference packs them — including its padding loop,
 * which leaves the last 32 columns uncounted when ncols is a multiple of 32.  Per candidate: the masks of its nleaves rows and
 * a rooted binary topology of nleaves - 1 internal nodes, children[2k], children[2k + 1] the two children of internal node k
 * (ids below nleaves are rows, nleaves + m is internal node m < k: post-order, the last one is the root); each id is a child
 * once.  scores[i] = the exact count.  PGM_ERR_INVALID: nleaves < 2, ncols == 0, a child out of range or not in post-order. */
typedef struct pgm_parsimony_job {
    const uint64_t *masks;      /* nleaves x ceil(ncols / 64) words */
    const uint32_t *children;   /* 2 * (nleaves - 1) */
    uint32_t nleaves, ncols;
} pgm_parsimony_job;
int pgm_gap_parsimony_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_parsimony_job *jobs, uint32_t *scores);
float pgm_parsimony_last_kernel_ms(pgm_ctx *ctx);

/* ---- weighted least-squares guide-tree refinement (reference src/LeastSquares.cpp) --------------------------------- */
/* pgm_wls_load keeps an n x n distance matrix D and weight matrix W (row-major, entry (k, l) at k * n + l) on the device,
 * in fp64, until the next load or pgm_ctx_destroy.  2 <= n <= PGM_WLS_MAX_N. */
#define PGM_WLS_MAX_N 32768
int pgm_wls_load(pgm_ctx *ctx, uint32_t n, const double *D, const double *W);

/* The subtree pair sums of LeastSquares.cpp:309-325 for many edges in one call.  A job splits the leaves into nsub subtrees
 * (4 around an edge, 5 around a quintet): label[l] is the subtree of leaf l (0..nsub-1) or -1, offset[l] the path length from
 * leaf l to its subtree's root.  For every pair of subtrees p < q, pair index s in lexicographic order ((0,1), (0,2), ...):
 *   out[PGM_WLS_OUT * j + s]      = sum over k in p, l in q of W(k,l) * ((D(k,l) - offset[k]) - offset[l])
 *   out[PGM_WLS_OUT * j + 10 + s] = sum over k in p, l in q of W(k,l)
 * and 0 in the slots past nsub (nsub - 1) / 2.  Each term takes the reference's operations, rounded to nearest, without
 * contraction; the terms are added in the fixed order of DESIGN.md ("WLS refinement"), the same in every call, so the host
 * statement of that order (Backend::wls_pair_sums_batch) gives the same bits.  PGM_ERR_INVALID: nothing loaded, nsub not 4
 * or 5, a label outside [-1, nsub), a NULL pointer. */
#define PGM_WLS_OUT 20
typedef struct pgm_wls_job {
    const int8_t *label;     /* n entries */
    const double *offset;    /* n entries (read where label >= 0) */
    uint32_t nsub;
} pgm_wls_job;
int pgm_wls_pair_sums_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_wls_job *jobs, double *out);
float pgm_wls_last_kernel_ms(pgm_ctx *ctx);       /* device time of the last pair-sums call */
uint32_t pgm_wls_last_launches(pgm_ctx *ctx);     /* kernels it launched */

/* ---- BioNJ guide trees (reference src/TreeNJ.cpp:132-281) ------------------------------------------------------------ */
/* The joins of BioNJ on the device: every value is the expression of the host loop (bionj_joins_host, host/bionj.cpp), the
 * column sums in Eigen's association, the joined pair the first strict minimum of the criterion in column-major order, so the
 * join record and final_d equal the host's bit for bit.  Three kernels per join of the largest family.
 * PGM_ERR_INVALID, before anything is launched: a NULL pointer, nfam == 0, a family with n < 4 or n > PGM_BIONJ_MAX_N, an
 * entry of D or V that is not finite. */
typedef struct pgm_bionj_join { uint32_t index1, index2; double dist1, dist2; } pgm_bionj_join;
#define PGM_BIONJ_MAX_N 32768
/* D, V: n x n row-major (entry (i,j) at i*n+j), as DistanceMatrix holds them; not modified.
 * joins: n-3 records in join order (reduced indices, index1 < index2, as buildNJTree uses them);
 * final_d: the 3 x 3 row-major D of the three clusters left, as the host's last formula reads it. */
int pgm_bionj(pgm_ctx *ctx, uint32_t n, const double *D, const double *V, pgm_bionj_join *joins, double *final_d);
/* nfam matrices back to back (n[f]^2 doubles each), joins back to back (n[f]-3 each), final_d 9 per family */
int pgm_bionj_multi(pgm_ctx *ctx, uint32_t nfam, const uint32_t *n, const double *D, const double *V,
                    pgm_bionj_join *joins, double *final_d);
uint32_t pgm_bionj_last_launches(pgm_ctx *ctx);   /* kernels of the last call */
float pgm_bionj_last_kernel_ms(pgm_ctx *ctx);     /* device time from its first kernel to its last */

/* The same joins when the pair of every join is known beforehand (--topology: branch lengths on a fixed topology; reference
 * src/TreeNJ.cpp:31-130, :158-179).  plan: n[f]-3 pairs per family back to back like joins, in reduced indices; join s of a
 * family joins plan[s] and evaluates no criterion, so it needs two column sums and costs O(n).  One preparation kernel, then one
 * kernel in which a workgroup per family runs all of the family's joins: the number of launches does not depend on n.  joins and
 * final_d as above; the values are those of bionj_joins_host with the same plan, bit for bit.
 * PGM_ERR_INVALID, before anything is launched: whatever pgm_bionj_multi rejects, a NULL plan, a pair with index1 >= index2 or
 * index2 >= n[f]-s at join s. */
typedef struct pgm_bionj_pair { uint32_t index1, index2; } pgm_bionj_pair;
int pgm_bionj_plan(pgm_ctx *ctx, uint32_t n, const double *D, const double *V, const pgm_bionj_pair *plan,
                   pgm_bionj_join *joins, double *final_d);
int pgm_bionj_plan_multi(pgm_ctx *ctx, uint32_t nfam, const uint32_t *n, const double *D, const double *V,
                         const pgm_bionj_pair *plan, pgm_bionj_join *joins, double *final_d);

/* ---- residue-pair agreement between a base alignment and nrep replicate alignments of the same sequences (pgmsa --guidance).
 * where[(r * nrows + i) * ncols + c]: the column of replicate r that holds the residue row i has in base column c, negative where
 * row i has a gap there.  With hit(r,i,j,c) = where[r][i][c] >= 0 && where[r][i][c] == where[r][j][c]:
 *   res_hits[i * ncols + c]  = sum over r and j != i of hit     (how often the residue's column-mates were recovered)
 *   pair_hits[i * nrows + j] = sum over r and c of hit, i != j  (symmetric, zero diagonal)
 * Both outputs are overwritten.  Two gaps never hit.  All sums are integers, so the results do not depend on the launch.
 * PGM_ERR_INVALID, before anything is launched or any buffer is touched: nrows, ncols or nrep zero, nrep * (nrows - 1) or
 * nrep * ncols beyond 32 bits (the range of the sums), more than 2^31 - 1 tiles of 64 x 64; then a null pointer. */
int pgm_msa_agreement(pgm_ctx *ctx, uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where,
                      uint32_t *res_hits /* nrows x ncols */, uint32_t *pair_hits /* nrows x nrows */);
float pgm_agreement_last_kernel_ms(pgm_ctx *ctx);   /* device time of the two kernels of the last call */

/* ---- transfer indices of the bipartitions of a tree against those of nrep replicate trees (pgmsa --bootstrap_tbe; Lemoine et al.,
 * Nature 2018).  A bipartition of nleaves leaves is a bit set of words = (nleaves + 63) / 64 little-endian uint64 words, either of its
 * sides, bits at or above nleaves zero.  With |A| = popcount, p(A) = min(|A|, nleaves - |A|) and the transfer distance
 * d(A, B) = min(h, nleaves - h), h = popcount(A xor B):
 *   phi[e * nrep + r] = min(p(A_e) - 1, min over rep_off[r] <= s < rep_off[r + 1] of d(A_e, B_s))
 * for reference set e (ref + e * words) and the sets B_s (rep + s * words) of replicate r.  p(A_e) - 1 is what the single-leaf
 * bipartitions of any tree give, so rep holds a replicate's other bipartitions only and may hold none.  phi is overwritten.
 * All values are integers, so the result does not depend on the launch.
 * PGM_ERR_INVALID, before anything is launched or phi is touched: nleaves < 4, nref == 0, nrep == 0, nref * nrep beyond 32 bits, a
 * null pointer (rep may be null when rep_off[nrep] == 0), rep_off not ascending from 0, a set with a bit at or above nleaves, a
 * reference set that is empty or full. */
int pgm_transfer_min(pgm_ctx *ctx, uint32_t nleaves, uint32_t nref, const uint64_t *ref /* nref x words */,
                     uint32_t nrep, const uint32_t *rep_off /* nrep + 1, ascending, rep_off[0] == 0 */,
                     const uint64_t *rep /* rep_off[nrep] x words */, uint32_t *phi /* nref x nrep, overwritten */);
float pgm_transfer_last_kernel_ms(pgm_ctx *ctx);   /* device time of the kernel(s) of the last pgm_transfer_min / pgm_transfer_taxa call */

/* ---- which taxa the transfer indices move (pgmsa --bootstrap_taxa: the taxon side of the transfer bootstrap).  Sets, p, h and
 * phi as for pgm_transfer_min.  The moved set T(A, B) is A xor B if h <= nleaves - h and else its complement within the nleaves
 * leaves: the leaves on the wrong side, |T| = d(A, B).
 *   arg[e * nrep + r]   = the lowest s in rep_off[r] <= s < rep_off[r + 1] with d(A_e, B_s) == phi[e * nrep + r], or
 *                         PGM_TRANSFER_NONE when no set of the replicate is that near (only the clamp p - 1 gave phi);
 *   (e, r) is counted   iff arg != PGM_TRANSFER_NONE and phi[e * nrep + r] <= thr[e];
 *   moved[e * nleaves + t] = the number of counted r whose T(A_e, B_arg) holds leaf t;  counted[e] = the number of counted r.
 * All four outputs are overwritten; all values are integers, so the result does not depend on the launch.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_transfer_min refuses, a null thr or output,
 * nleaves beyond 2^31 - 1, nref * nleaves beyond 32 bits.  thr is otherwise free (0xffffffff counts every pair with a set). */
#define PGM_TRANSFER_NONE 0xffffffffu
int pgm_transfer_taxa(pgm_ctx *ctx, uint32_t nleaves, uint32_t nref, const uint64_t *ref /* nref x words */, const uint32_t *thr /* nref */,
                      uint32_t nrep, const uint32_t *rep_off /* nrep + 1 */, const uint64_t *rep /* rep_off[nrep] x words */,
                      uint32_t *phi /* nref x nrep */, uint32_t *arg /* nref x nrep */, uint32_t *moved /* nref x nleaves */,
                      uint32_t *counted /* nref */);

/* ---- likelihood of an alignment on a rooted tree, with the first and second derivative of its logarithm by every branch length
 * (pgmsa --ml_tree; Felsenstein pruning).
 * The tree: nnodes nodes, children before parents (parent[v] > v), the leaves are nodes 0 .. nleaves-1, the root is the one node
 * whose parent is UINT32_MAX; a node's children are taken in ascending node order and an inner node has at least two.  Edge e is
 * the edge above node e (e < nnodes-1: the root is the last node).
 * rows[l * ncols + s]: leaf l at site s, 0 .. dim-1 a state, -1 a gap, -2 a residue without a value (both: missing data).
 * P: per edge e one dim x dim matrix (derivs == 0) or three back to back (P, P' = Q P, P'' = Q Q P), column-major, X(i, j) at
 * i + dim * j = parent state i -> child state j.  All matrices are the caller's: no transcendental function runs on the device.
 *   up     U_l(j) = 1 if rows == j or rows < 0, else 0;  U_v(i) = prod over the children c of S_c(i), S_c(i) = sum_j P_c(i, j) U_c(j)
 *   scale  after a node's product: if the largest of its dim entries is below 2^-256 and above 0, every entry * 2^256, site_k += 1
 *   site   site_l[s] = sum_i pi[i] U_root(i); the likelihood of the site is site_l[s] * 2^(-256 site_k[s])
 *   down   O_c(i) = B_v(i) * prod over the siblings c' of c of S_c'(i), v the parent of c, B_root = pi,
 *          B_v(i) = sum_h O_v(h) P_v(h, i); then the scaling rule (no count: only ratios are taken)
 *   edge   A^X = sum_i O_e(i) * (sum_j X_e(i, j) U_e(j)) for X = P, P', P'';  g = A^P' / A^P,  h = A^P'' / A^P - g * g
 *   d1[e] = sum_s g, d2[e] = sum_s h: sites ascending within consecutive chunks of PGM_TREELIK_CHUNK sites, then the chunk sums
 *          ascending.
 * Every sum runs over its index ascending and starts from 0.0 with one multiply and one add per term; every product starts with its
 * first factor.  Only + - * / occur and nothing is contracted, so the values do not depend on the launch and equal the host
 * statement's (tree_likelihood_host) bit for bit.  site_l and site_k are overwritten; d1 and d2 (nnodes-1 each) only when derivs.
 * Stateless: everything is uploaded per call.  Device memory: 8 * (nnodes - nleaves) * ncols * dim bytes for the partials, as much
 * again and 16 * (nnodes - 1) * ncols for the per-site ratios with derivs (below the round figure 2 * nnodes * ncols * dim * 8);
 * memory that cannot be had is PGM_ERR_NOMEM.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: a null pointer (d1, d2 only when derivs), dim outside
 * 1 .. 64, nleaves < 2, ncols == 0, nnodes <= nleaves, a parent index <= its child or >= nnodes, a leaf that is a parent, an inner
 * node with fewer than 2 children, not exactly one root, a row value outside -2 .. dim-1. */
#define PGM_TREELIK_CHUNK 16
int pgm_tree_likelihood(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent /* nnodes, root: UINT32_MAX */,
                        uint32_t ncols, const int8_t *rows /* nleaves x ncols */, const double *pi /* dim */,
                        const double *P /* (nnodes-1) x {1 or 3} x dim x dim */, int derivs,
                        double *site_l /* ncols */, int32_t *site_k /* ncols */, double *d1, double *d2 /* nnodes-1, derivs only */);
float pgm_treelik_last_kernel_ms(pgm_ctx *ctx);   /* device time of the kernels of the last pgm_tree_likelihood, pgm_tree_likelihood_rates, pgm_tree_ancestral, pgm_tree_nni, pgm_tree_nni_edge, pgm_tree_spr, pgm_tree_ancestral_joint or pgm_tree_ancestral_sample call */

/* ---- the same likelihood under a mixture of ncat rate categories (pgmsa --ml_tree --ml_gamma).
 * Everything from dim to pi, and derivs, d1, d2, is as in pgm_tree_likelihood, with the same checks.  ncat: 1 .. PGM_TREELIK_MAXCAT;
 * w: the ncat weights, each finite and > 0; P: ncat x (nnodes-1) x {3 or 1} x dim x dim, category-major, every matrix column-major as
 * above.  The device sees no rates: the caller folds them into the matrices (P(r_c t_e), r_c Q P, r_c^2 Q Q P).
 * Per category c the up pass, the scaling rule, the down pass and the three sums A^P, A^P', A^P'' of every edge are those of
 * pgm_tree_likelihood; they give (L_c, k_c) per site and per edge and site g_c = A^P' / A^P and q_c = A^P'' / A^P (no - g g yet).
 * Then per site, in this order:
 *   site_k = min_c k_c
 *   term_c = w_c * L_c, then multiplied by 2^-256 exactly (k_c - site_k) times
 *   site_l = sum_c term_c, c ascending from 0.0;   post[c * ncols + s] = term_c / site_l
 *   per edge  g = sum_c post_c * g_c,  q = sum_c post_c * q_c  (c ascending from 0.0, one multiply and one add per term),  h = q - g * g
 *   d1, d2: the chunk sums of g and h as above.
 * With ncat == 1 and w = {1.0} every output equals pgm_tree_likelihood's bit for bit (1.0 * x and 0.0 + x are exact, x / x is 1.0),
 * and post is 1.0.  The values do not depend on the launch and equal the host statement's (tree_likelihood_rates_host) bit for bit.
 * site_l, site_k and post (ncat x ncols) are overwritten; d1 and d2 only when derivs.  Device memory: ncat times that of
 * pgm_tree_likelihood and 16 * (nnodes - 1) * ncols more; memory that cannot be had is PGM_ERR_NOMEM.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_likelihood refuses, ncat outside
 * 1 .. PGM_TREELIK_MAXCAT, a null w or post, a w entry that is not finite and > 0. */
#define PGM_TREELIK_MAXCAT 16
int pgm_tree_likelihood_rates(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                              const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x {1 or 3} x dim x dim */,
                              int derivs, double *site_l /* ncols */, int32_t *site_k /* ncols */, double *post /* ncat x ncols */,
                              double *d1, double *d2 /* nnodes-1, derivs only */);

/* ---- marginal ancestral states on the same tree under the same mixture (pgmsa --ml_tree --ml_ancestral).
 * Everything from dim to w is as in pgm_tree_likelihood_rates, with the same checks; P: ncat x (nnodes-1) x dim x dim, P alone (the
 * derivs == 0 layout).  site_l, site_k and post are pgm_tree_likelihood_rates's values with derivs == 0, bit for bit: the same up
 * pass and the same combine order.  ninner = nnodes - nleaves; inner node v has row v - nleaves.
 * Per category c, per site, per inner node v:
 *   down   the down pass of pgm_tree_likelihood with S from P alone: B_root = pi, B_v(i) = sum_h O_v(h) P_v(h, i) (h ascending from
 *          0.0), O_child(i) = B_v(i) times the siblings' S(i) in ascending child order (the product starts with B_v(i)), then the
 *          scaling rule, without a count
 *   m(i) = B_v(i) * U_v(i), U_v the stored (scaled) partial;  Z = sum_i m(i), i ascending from 0.0;  a_c,v(i) = m(i) / Z, and 0.0 for
 *          every i when Z == 0.0
 * Then the mixture, anc(v, s, i) = sum_c post[c][s] * a_c,v(i), c ascending from 0.0, one multiply and one add per term:
 *   anc_post[((v - nleaves) * ncols + s) * dim + i] = anc   (only when anc_post is not null)
 *   anc_prob[(v - nleaves) * ncols + s] = the largest anc over i,  anc_state[...] = the smallest i that has it;
 *   when no anc is above 0.0: anc_state = -1, anc_prob = 0.0.
 * With ncat == 1 and w = {1.0} anc is a_0,v exactly (1.0 * x and 0.0 + x are exact).  Only + - * / occur and nothing is contracted:
 * the values do not depend on the launch and equal the host statement's (tree_ancestral_host) bit for bit.  Every output is
 * overwritten (anc_post only when given).  Device memory: ncat * 16 * ninner * ncols * dim bytes for the partials and the outside
 * vectors, in whose place the categories' posteriors are written (what pgm_tree_likelihood_rates takes with derivs, without its
 * per-edge ratios); the inputs, 8 * ncat * (nnodes-1) * dim * dim bytes of matrices and nleaves * ncols + 8 * nnodes + 8 * (dim +
 * ncat) bytes for the rows, the children lists, pi and w; 12 * ncat * ncols bytes for (L_c, k_c); and the outputs, (12 + 8 * ncat) *
 * ncols + 9 * ninner * ncols bytes, with anc_post 8 * ninner * ncols * dim more.  Memory that cannot be had is PGM_ERR_NOMEM.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_likelihood_rates refuses (derivs == 0), a null
 * anc_state or anc_prob. */
int pgm_tree_ancestral(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                       const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x dim x dim */,
                       double *site_l /* ncols */, int32_t *site_k /* ncols */, double *post /* ncat x ncols */,
                       int8_t *anc_state /* ninner x ncols */, double *anc_prob /* ninner x ncols */,
                       double *anc_post /* ninner x ncols x dim, or NULL */);

/* ---- the nearest-neighbour interchanges of the same tree under the same mixture (pgmsa --ml_tree --ml_search).
 * Everything from dim to P is as in pgm_tree_ancestral, with the same checks.  site_l, site_k and post are
 * pgm_tree_likelihood_rates's values with derivs == 0, bit for bit.
 * Candidate q = (v, a, c) = (cand_v[q], cand_a[q], cand_c[q]): v an inner node that is not the root, u = parent[v], a a child of v, c a
 * child of u other than v.  The neighbour tree has a and c exchanged: both keep their own edges and matrices, v keeps its own, the
 * root stays (rooted NNI; the parent -> child direction of every matrix is kept, so a generator need not be reversible).  Nodes of
 * any arity; a binary tree has two candidates per inner node below the root.
 * Per category k, site s and candidate, with S_x(i) = sum_j P_x(i, j) U_x(j) and the stored (scaled) partials U and outside vectors O
 * of the down pass of pgm_tree_ancestral (P alone):
 *   B_u(i) = pi[i] if u is the root, else sum_h O_u(h) P_u(h, i), h ascending from 0.0
 *   R(i) = B_u(i) times S_c'(i) of the children c' of u other than v and c, in child order (the product starts with B_u(i))
 *   T(j) = the product of S_b(j) over the children b of v other than a, in child order (the product starts with its first factor)
 *   for (x, y) = (a, c), the tree as it is: (D, k_D); for (x, y) = (c, a), the neighbour: (N, k_N):
 *     X(j) = T(j) * S_x(j), then the scaling rule on its dim values (largest below 2^-256 and above 0: times 2^256, count one)
 *     Y(i) = R(i) * S_y(i), then the same rule
 *     W(i) = sum_j P_v(i, j) X(j), j ascending from 0.0;   A = sum_i Y(i) * W(i), i ascending from 0.0;   k = the two counts added
 *   rho_k = 0.0 when D == 0.0, else N / D multiplied by 2^-256 exactly (k_N - k_D) times, or by 2^256 exactly (k_D - k_N) times
 *   rho[q * ncols + s] = sum_k post[k][s] * rho_k, k ascending from 0.0
 * N and D are multilinear in the same four scaled pieces, so the stored scale factors cancel: rho is the neighbour's site likelihood
 * over the current one, and the mixture with post is sum_k w_k L'_k / sum_k w_k L_k.  Only + - * / occur and nothing is contracted:
 * the values do not depend on the launch and equal the host statement's (tree_nni_host) bit for bit.  site_l, site_k, post and rho
 * are overwritten.  Device memory: ncat * 16 * ninner * ncols * dim bytes for the partials and the outside vectors; the inputs,
 * 8 * ncat * (nnodes-1) * dim * dim bytes of matrices and nleaves * ncols + 12 * nnodes + 12 * ncand + 8 * (dim + ncat) bytes for the
 * rows, the children lists, the parents, the candidates, pi and w; 12 * ncat * ncols bytes for (L_c, k_c); and the outputs,
 * (12 + 8 * ncat) * ncols + 8 * ncand * ncols bytes.  Memory that cannot be had is PGM_ERR_NOMEM.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_ancestral refuses (its own outputs aside),
 * ncand == 0, a null candidate array or rho, a candidate whose v is a leaf, the root or >= nnodes, parent[a] != v,
 * parent[c] != parent[v], c == v. */
int pgm_tree_nni(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                 const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x dim x dim */,
                 uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c /* ncand each */,
                 double *site_l /* ncols */, int32_t *site_k /* ncols */, double *post /* ncat x ncols */, double *rho /* ncand x ncols */);

/* ---- the same interchanges, each at a trial length of its own central edge, with the derivatives of its log-likelihood by that
 * length (pgmsa --ml_tree --ml_search / --ml_support with --ml_nni_opt).
 * Everything from dim to cand_c, and site_l, site_k, post, is as in pgm_tree_nni, with the same checks.  Pc: ncat x ncand x 3 x dim x
 * dim doubles, category-major, every matrix column-major: for category k and candidate q the three matrices P, P', P'' back to back
 * of the edge above v = cand_v[q] in the neighbour tree at that candidate's trial length, the category's rate folded in (P(r_k t),
 * r_k Q P, r_k^2 Q Q P: what pgm_tree_likelihood_rates reads for an edge with derivs).  The device sees no rates and no lengths.
 * Per category k, site s and candidate: B_u, R, T, S_a, S_c, X_D = T S_a, Y_D = R S_c, X_N = T S_c, Y_N = R S_a, the scaling rule, the
 * counts k_D and k_N, and D = sum_i Y_D(i) (sum_j P_v(i, j) X_D(j)) exactly as in pgm_tree_nni, P_v the tree's own matrix from P.  Then
 *   for Z = P, P', P'' of Pc[k][q]:  W^Z(i) = sum_j Z(i, j) X_N(j), j ascending from 0.0;  N^Z = sum_i Y_N(i) W^Z(i), i ascending from 0.0
 *   r^Z_k = 0.0 when D == 0.0, else N^Z / D multiplied by 2^-256 exactly (k_N - k_D) times, or by 2^256 exactly (k_D - k_N) times
 *   rho = sum_k post_k r^P_k,  G = sum_k post_k r^P'_k,  Q = sum_k post_k r^P''_k  (k ascending from 0.0, one multiply and one add per term)
 *   g = G / rho,  h = Q / rho - g * g;  both 0.0 when rho == 0.0
 *   rho[q * ncols + s] = rho;  d1[q] = sum_s g,  d2[q] = sum_s h: sites ascending within consecutive chunks of PGM_TREELIK_CHUNK sites,
 *   then the chunk sums ascending, as pgm_tree_likelihood sums an edge.
 * D and post do not depend on the trial length, so d1[q] and d2[q] are the first and second derivative of the neighbour's
 * log-likelihood by the length of its central edge, at the trial length.  Where the P block of Pc[k][q] equals P_v of category k, rho
 * equals pgm_tree_nni's bit for bit.  Only + - * / occur and nothing is contracted: the values do not depend on the launch and equal
 * the host statement's (tree_nni_edge_host) bit for bit.  site_l, site_k, post, rho, d1 and d2 (ncand each) are overwritten.
 * Device memory: that of pgm_tree_nni, and 24 * ncat * ncand * dim * dim bytes for Pc, 16 * ncand * ncols for the per-site ratios,
 * 16 * ncand * nchunks for the chunk sums (nchunks = ceil(ncols / PGM_TREELIK_CHUNK)) and 16 * ncand for d1 and d2.  Memory that
 * cannot be had is PGM_ERR_NOMEM.  pgm_treelik_last_kernel_ms covers the call.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_nni refuses, a null Pc, d1 or d2. */
int pgm_tree_nni_edge(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                      const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x dim x dim */,
                      uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c /* ncand each */,
                      const double *Pc /* ncat x ncand x 3 x dim x dim */, double *site_l /* ncols */, int32_t *site_k /* ncols */,
                      double *post /* ncat x ncols */, double *rho /* ncand x ncols */, double *d1, double *d2 /* ncand each */);

/* ---- subtree pruning and regrafting on the same tree under the same mixture (pgmsa --ml_tree --ml_search --ml_spr).
 * Everything from dim to P is as in pgm_tree_nni, with the same checks; site_l, site_k and post are pgm_tree_likelihood_rates's values
 * with derivs == 0, bit for bit.  Ph: the shape of P, per category and edge the matrix of HALF that edge (the caller's choice of
 * half; the category's rate folded in).  The device sees no lengths or rates and runs no transcendental function.
 * Candidate q = (v, y) = (cand_v[q], cand_y[q]) prunes the subtree below v, with the edge above v and its matrix P_v, from
 * p = parent[v], and regrafts it on the edge above y: that edge gets a new node n in its middle, both halves with Ph_y, the children
 * of n are y and v.  The root stays and every matrix keeps its parent -> child direction (a generator need not be reversible).  Where
 * p is left with one child s it is kept as a node of one child: P_p P_s is the matrix of the joined edge (Chapman-Kolmogorov).
 * Valid: v and y are not the root, y is not in the subtree of v (v itself included), p is not a root of exactly two children, and
 * where p has exactly two children y is neither p nor the sibling of v (both give the tree itself).
 * The path: a the lowest common ancestor of p and y (a node is its own ancestor); up a_0 = p, a_1 = parent[a_0], .., a_J = a; down
 * a = c_0, c_1, .., c_M = y (M == 0: y is p or an ancestor of p); J + M <= PGM_TREE_SPR_MAXPATH edges.
 * Per category k, site s and candidate, with S_x(i) = sum_j P_x(i, j) U_x(j) (the leaf rule for U), the stored scaled U and O of
 * pgm_tree_nni, and the scaling rule with a count (largest of a vector's dim values below 2^-256 and above 0: the vector times 2^256,
 * the count plus one).  Two chains, - without v and + with it, each with its own count k- or k+:
 *   start (only where J >= 1 or M == 0): E-_0(i) = the product of S_c(i) over the children c of p other than v, in child order (it
 *     starts with its first factor); E+_0(i) = E-_0(i) * S_v(i) (from the unscaled E-_0); the rule on each
 *   up, j = 1 .. J: Mup(+-)(i) = sum_l P_{a_{j-1}}(i, l) E(+-)_{j-1}(l), l ascending from 0.0; if j < J or M == 0:
 *     E(+-)_j(i) = Mup(+-)(i) times S_c(i) of the children c of a_j other than a_{j-1}, in child order (it starts with Mup); the rule
 *   M == 0, the target on the up chain: Z(m) = sum_j Ph_y(m, j) E-_J(j); X(m) = S_v(m) * Z(m), the rule, counted into k-;
 *     W(h) = sum_m Ph_y(h, m) X(m); N = sum_h O_y(h) * W(h); D = sum_h O_y(h) * (sum_j P_y(h, j) E+_J(j))
 *   M >= 1, the turn: B_a(i) = pi[i] at the root, else sum_h O_a(h) P_a(h, i), h ascending from 0.0.  J >= 1: G(+-)_1(i) = B_a(i) *
 *     Mup(+-)(i) (the Mup of j = J), times S_c(i) of the children c of a other than a_{J-1} and c_1, in child order.  J == 0:
 *     G-_1(i) = B_a(i) times S_c(i) of the children of a other than v and c_1, in child order; G+_1(i) = G-_1(i) * S_v(i), before
 *     either is scaled.  The rule on each.
 *   down, m = 1 .. M - 1: Bc(+-)(i) = sum_h G(+-)_m(h) P_{c_m}(h, i), h ascending from 0.0; G(+-)_{m+1}(i) = Bc(+-)(i) times S_c(i) of
 *     the children of c_m other than c_{m+1}, in child order; the rule
 *   the target below the turn: Z(m) = sum_j Ph_y(m, j) U_y(j) (the leaf rule); X(m) = S_v(m) * Z(m), the rule into k-;
 *     W(h) = sum_m Ph_y(h, m) X(m); N = sum_h G-_M(h) * W(h); D = sum_h G+_M(h) * S_y(h)
 *   rho_k = 0.0 when D == 0.0, else N / D multiplied by 2^-256 exactly (k- - k+) times, or by 2^256 exactly (k+ - k-) times
 *   rho[q * ncols + s] = sum_k post[k][s] * rho_k, k ascending from 0.0
 * N and D are multilinear in the same stored pieces, so their unknown scale factors cancel: rho is the regrafted tree's site
 * likelihood over the tree's own.  Every sum runs ascending from 0.0 with one multiply and one add per term, only + - * / occur and
 * nothing is contracted: the values do not depend on the launch or on the order of the candidates and equal the host statement's
 * (tree_spr_host) bit for bit.  site_l, site_k, post and rho are overwritten.
 * Device memory: that of pgm_tree_nni without its candidates, and 8 * ncat * (nnodes-1) * dim * dim bytes for Ph,
 * (4 + 4 * (PGM_TREE_SPR_MAXPATH + 4)) * ncand bytes for the candidates and their paths.  Memory that cannot be had is PGM_ERR_NOMEM.
 * pgm_treelik_last_kernel_ms covers the call.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_nni refuses of the arguments they share, a null
 * Ph, cand_v, cand_y or rho, ncand == 0, a candidate that is not valid, a path of more than PGM_TREE_SPR_MAXPATH edges. */
#define PGM_TREE_SPR_MAXPATH 16
int pgm_tree_spr(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                 const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x dim x dim */,
                 const double *Ph /* as P: the matrix of half of every edge */, uint32_t ncand, const uint32_t *cand_v,
                 const uint32_t *cand_y /* ncand each */, double *site_l /* ncols */, int32_t *site_k /* ncols */,
                 double *post /* ncat x ncols */, double *rho /* ncand x ncols */);

/* ---- the jointly most probable ancestral states on the same tree under the same mixture (pgmsa --ml_tree --ml_ancestral_joint;
 * Pupko et al. 2000).
 * Everything from dim to P is as in pgm_tree_ancestral, with the same checks; site_l, site_k and post are pgm_tree_likelihood_rates's
 * values with derivs == 0, bit for bit: the same up pass and the same combine.  ninner = nnodes - nleaves; inner node v has row
 * v - nleaves.  Per site s:
 *   cat[s] = the smallest k whose post[k][s] is the largest (k ascending from 0; a later k takes over only when strictly greater).  The
 *          joint assignment is taken under that category: the arg-max over the assignments of the whole mixture does not decompose
 *          over the tree and is not computed.
 *   With the matrices of category cat[s], a max-product up pass over the inner nodes ascending:
 *   leaf   m_c(i) = S_c(i) of pgm_tree_likelihood: 0.0 + P_c(i, r) for a leaf of state r, the sum of P_c(i, j) over j ascending from 0.0
 *          for missing data
 *   F_v(j) = the product of m_c(j) over the children c of v in child order (it starts with its first factor); then the scaling rule
 *          on its dim values (largest below 2^-256 and above 0: every value * 2^256, joint_k += 1)
 *   v not the root:  m_v(i) = max_j P_v(i, j) * F_v(j): one multiply per term, j ascending, the maximum starts as the term of j = 0 and
 *          a later term replaces it only when strictly greater;  ptr_v(i) = the j that holds it (the smallest such j)
 *   root   r(j) = pi[j] * F_root(j);  joint_l[s] = the maximum of r by the same rule, the root's state the j that holds it
 *   back   the inner nodes below the root descending (parents first): state(v) = ptr_v(state(parent[v]))
 *   joint_state[(v - nleaves) * ncols + s] = state(v);  every state of the site is -1 when joint_l[s] == 0.0
 * joint_l * 2^(-256 joint_k) is the probability of the column together with that assignment under category cat[s].  Only * and
 * comparisons occur past the leaves' sums and nothing is contracted: the values do not depend on the launch and equal the host
 * statement's (tree_ancestral_joint_host) bit for bit.  Every output is overwritten.
 * Device memory: that of pgm_tree_likelihood_rates with derivs == 0 (ncat * 8 * ninner * ncols * dim bytes of partials, the inputs,
 * 12 * ncat * ncols for (L_c, k_c), (12 + 8 * ncat) * ncols of outputs), and 8 * ninner * ncols * dim bytes for F, ninner * ncols * dim
 * for the back-pointers, (13 + ninner) * ncols for cat, joint_l, joint_k and joint_state.  Memory that cannot be had is PGM_ERR_NOMEM.
 * pgm_treelik_last_kernel_ms covers the call.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_ancestral refuses (its own outputs aside), a null
 * cat, joint_state, joint_l or joint_k. */
int pgm_tree_ancestral_joint(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                             const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x dim x dim */,
                             double *site_l /* ncols */, int32_t *site_k /* ncols */, double *post /* ncat x ncols */, uint8_t *cat /* ncols */,
                             int8_t *joint_state /* ninner x ncols */, double *joint_l /* ncols */, int32_t *joint_k /* ncols */);

/* ---- ancestral states drawn from their joint posterior on the same tree under the same mixture (pgmsa --ml_tree
 * --ml_ancestral_samples; the stochastic traceback through the partials).
 * Everything from dim to P, and site_l, site_k, post, is as in pgm_tree_ancestral_joint, with the same checks.  The call writes the
 * samples N = first_sample + n, n = 0 .. nsamp - 1; what a sample holds depends on N, the site and seed alone, so a caller may cut its
 * samples into calls of bounded output.
 * Draw x of sample N at site s (x = 0: the category; x = 1 + (v - nleaves): inner node v), all integer arithmetic mod 2^64:
 *   z = splitmix64 of the state seed + 0x9E3779B97F4A7C15 * (((N * ncols) + s) * (ninner + 1) + x), that is
 *       z = state + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 *   u = (z >> 11) * 2^-53   (exact: 0 <= u < 1)
 * The pick of a draw on the weights q_0 .. q_{m-1}:
 *   T = the sum of the weights, ascending from 0.0;  T == 0.0: the pick is -1
 *   target = u * T;  c = 0.0, then c = c + q_j for j ascending: the pick is the first j with c > target;  when there is none (a NaN
 *   among the weights; with finite weights u * T is below T, where c ends) the largest j with q_j > 0, and -1 when there is none either
 * The weights:
 *   category   post[k][s], k = 0 .. ncat - 1
 *   root, in the picked category k:   pi[i] * U_root(i), U the stored scaled partials of category k at the site
 *   node v below the root, descending (parents first), its parent in state i:   P_v(i, j) * U_v(j), the matrix and partial of category k
 *   a category of -1 or a parent of -1 gives -1
 * The scale factors of the partials cancel in target / T: every draw is from the exact conditional distribution, so a sample is an
 * independent draw from the posterior of (category, every inner state) given the column.
 *   samp_cat[s * nsamp + n] = the category (255 for -1);   samp_state[((v - nleaves) * ncols + s) * nsamp + n] = the state of v
 * A weight is formed by one multiply wherever it is needed, every sum runs ascending from 0.0 with one add per term and nothing is
 * contracted: the values do not depend on the launch and equal the host statement's (tree_ancestral_sample_host) byte for byte.  Every
 * output is overwritten.
 * Device memory: that of pgm_tree_likelihood_rates with derivs == 0, and (1 + ninner) * ncols * nsamp bytes for the samples.  Memory
 * that cannot be had is PGM_ERR_NOMEM.  pgm_treelik_last_kernel_ms covers the call.
 * PGM_ERR_INVALID, before anything is launched or an output is touched: what pgm_tree_ancestral refuses (its own outputs aside),
 * nsamp == 0, a null samp_cat or samp_state. */
int pgm_tree_ancestral_sample(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                              const double *pi, uint32_t ncat, const double *w /* ncat */, const double *P /* ncat x (nnodes-1) x dim x dim */,
                              uint32_t nsamp, uint64_t first_sample, uint64_t seed, double *site_l /* ncols */, int32_t *site_k /* ncols */,
                              double *post /* ncat x ncols */, uint8_t *samp_cat /* ncols x nsamp */, int8_t *samp_state /* ninner x ncols x nsamp */);

/* The sums of every row of a matrix over nrep resamplings of its columns (`pgmsa --ml_tree --ml_support`): with
 * x = log rho of pgm_tree_nni, the resampled log-likelihood gain of every neighbour of the tree in every bootstrap replicate.
 *   out[q * nrep + r] = sum over k of x[q * ncols + cols[r * ncols + k]], k ascending from 0.0
 * Every step is one IEEE fp64 addition: no multiplication, no contraction, no pairwise or tree order.  The values therefore do not
 * depend on the launch and equal the host statement's (resampled_sums_host) bit for bit.  Entries of -infinity are allowed and
 * propagate (-infinity + finite = -infinity).  The caller must pass neither a NaN nor +infinity: this is NOT checked.  cols is laid out
 * as pgm_prealigned_counts_resampled reads it.  out is overwritten.
 * Device memory: 8 * nrow * ncols bytes for x and 8 * ceil(nrow / 64) * 64 * ncols for its transpose, 4 * nrep * ncols for cols and
 * 8 * nrow * nrep for out.  Memory that cannot be had is PGM_ERR_NOMEM.
 * PGM_ERR_INVALID, before anything is launched or out is touched: a null pointer, nrow, ncols or nrep == 0, nrow * nrep or
 * nrep * ncols beyond 32 bits, a cols entry >= ncols. */
int pgm_resampled_sums(pgm_ctx *ctx, uint32_t nrow, uint32_t ncols, const double *x /* nrow x ncols, row-major */, uint32_t nrep,
                       const uint32_t *cols /* nrep x ncols */, double *out /* nrow x nrep */);
float pgm_resample_last_kernel_ms(pgm_ctx *ctx);   /* device time of the two kernels of the last pgm_resampled_sums call */

#ifdef __cplusplus
}
#endif
#endif /* PGM_HIP_H_ */
