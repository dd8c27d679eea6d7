// backend_hip.cpp — binds the host call surface to libpgm_hip.so (the HIP kernels behind the C ABI
// of include/pgm_hip.h).  There is deliberately no CPU fallback: without a usable MI355X context
// every hot-path call fails loudly.
#include "pgm_host.h"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace pgm {
namespace {
struct HipBackend : Backend {
    // One context per device.  PGM_DEVICES="0,2,5" lists them explicitly, PGM_DEVICE=k selects one (what a one-process-
    // per-GPU launcher sets), otherwise every visible device is used.  Every batch call runs on the context the caller names
    // (`worker`): the host code deals a batch's independent units — jobs of a guide-tree level, leaves, merges, sequence
    // pairs — to the contexts, one host thread each (farm_shards / computePwDistances).
    std::vector<pgm_ctx *> ctxs;
    std::vector<const CSProfile *> loaded;   // the profile library resident on context w
    // Two contexts on ONE device (PGM_DEVICES=0,0: a test set-up) must not run their alignGraphs batches at the same time: every
    // batch sizes its persistent grids for the whole device (no grid of a stage waits for a CU).  One lock per device.
    std::map<int, std::unique_ptr<std::mutex>> device_lock;
    std::vector<int> device_of;
    HipBackend() {
        std::vector<int> devs;
        if (const char *e = getenv("PGM_DEVICES")) {
            for (const char *p = e; *p;) { devs.push_back(atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
        } else if (const char *e = getenv("PGM_DEVICE")) {
            devs.push_back(atoi(e));
        } else {
            const int n = pgm_device_count();
            for (int d = 0; d < std::max(n, 1); ++d) devs.push_back(d);
        }
        for (int d : devs) {
            pgm_ctx *c = nullptr;
            if (pgm_ctx_create(d, &c) != PGM_OK || !c)
                error("libpgm_hip: cannot create a context on device %d: %s", d, pgm_last_error());
            ctxs.push_back(c);
            device_of.push_back(d);
            if (!device_lock.count(d)) device_lock[d].reset(new std::mutex);
        }
        loaded.assign(ctxs.size(), nullptr);
    }
    pgm_ctx *ctx_of(int worker) const { return ctxs[(size_t)worker % ctxs.size()]; }
    ~HipBackend() override { for (pgm_ctx *c : ctxs) pgm_ctx_destroy(c); }
    const char *name() const override { return "hip"; }
    int workers() const override { return (int)ctxs.size(); }
    void align_graphs_batch(uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                            const pgm_model *const *model, const pgm_scores *scores, pgm_align_out *out, int worker,
                            const pgm_site_ref *res1, const pgm_site_ref *res2) override {
        std::lock_guard<std::mutex> one_batch_per_device(*device_lock.at(device_of[(size_t)worker % ctxs.size()]));
        int rc = pgm_align_graphs_batch_res(ctx_of(worker), njobs, g1, g2, model, scores, res1, res2, out);
        if (rc != PGM_OK && rc != PGM_ERR_BACKTRACK) error("pgm_align_graphs_batch failed (%d): %s", rc, pgm_last_error());
    }
    // resident profiles (PGM_NO_RESIDENT switches them off): with several contexts the pass is sharded by subtree and the few matrices
    // a parent needs from another device are copied over (progressive.cpp assign_owners, resident_import)
    bool resident() const override { return !host_switches().no_resident; }
    const double *resident_import(int dst, int src, const double *p, size_t count) override {
        const double *out = nullptr;
        int rc = pgm_resident_import(ctx_of(dst), ctx_of(src), p, (uint64_t)count, &out);
        if (rc != PGM_OK) error("pgm_resident_import failed (%d): %s", rc, pgm_last_error());
        return out;
    }
    bool resident_onehot(uint32_t dim, uint32_t nseq, const int8_t *syms, const uint32_t *offs, const double **dev, int worker) override {
        int rc = pgm_resident_onehot(ctx_of(worker), dim, nseq, syms, offs, dev);
        if (rc != PGM_OK) error("pgm_resident_onehot failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    void resident_reset() override { for (pgm_ctx *c : ctxs) (void)pgm_resident_reset(c); }
    bool merge_profiles_batch_res(uint32_t njobs, const pgm_merge_job *jobs, const double **dev, int worker) override {
        int rc = pgm_merge_profiles_batch_ex(ctx_of(worker), njobs, jobs, PGM_MERGE_RESIDENT, dev);
        if (rc != PGM_OK) error("pgm_merge_profiles_batch_ex failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    int nw_pairs_submit(uint32_t dim, const int32_t *score, int32_t go, int32_t ge, uint32_t nseq, const int8_t *syms,
                        const uint32_t *offs, uint32_t npairs, const uint32_t *pi, const uint32_t *pj, uint32_t flags, int32_t *counts,
                        uint32_t *gaps, int worker) override {
        int ticket = -1;
        int rc = pgm_nw_pairs_submit(ctxs[(size_t)worker % ctxs.size()], dim, score, go, ge, nseq, syms, offs, npairs, pi, pj, flags, counts, gaps, &ticket);
        if (rc != PGM_OK) error("pgm_nw_pairs_submit failed (%d): %s", rc, pgm_last_error());
        return ticket;
    }
    void nw_pairs_wait(int ticket, int worker) override {
        int rc = pgm_nw_pairs_wait(ctxs[(size_t)worker % ctxs.size()], ticket);
        if (rc != PGM_OK) error("pgm_nw_pairs_wait failed (%d): %s", rc, pgm_last_error());
    }
    void *host_alloc(size_t bytes) override {
        void *p = pgm_host_alloc(bytes);
        if (!p) error("pgm_host_alloc(%zu) failed", bytes);
        return p;
    }
    void host_free(void *p) override { pgm_host_free(p); }
    bool mldist_batch(const pgm_mldist_model &m, uint32_t npairs, const int32_t *counts, const uint32_t *gaps, const double *seqlen,
                      double *dist, double *var, int worker) override {
        int rc = pgm_mldist_batch(ctxs[(size_t)worker % ctxs.size()], &m, npairs, counts, gaps, seqlen, dist, var);
        if (rc != PGM_OK) error("pgm_mldist_batch failed (%d): %s", rc, pgm_last_error());
        mldist_device_pairs += npairs;
        mldist_kernel_ms += pgm_dist_last_kernel_ms(ctxs[(size_t)worker % ctxs.size()]);
        return true;
    }
    bool mldist_general() const override { return true; }
    bool prealigned_counts_batch(uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t npairs, const uint32_t *pi,
                                 const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) override {
        int rc = pgm_prealigned_counts_batch(ctx_of(worker), dim, nrows, ncols, rows, npairs, pi, pj, counts, gaps);
        if (rc != PGM_OK) error("pgm_prealigned_counts_batch failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    void kmer_cosine(uint32_t nseq, uint32_t ncols, const int32_t *counts, double *cosine, int worker) override {
        int rc = pgm_kmer_cosine(ctx_of(worker), nseq, ncols, counts, cosine);
        if (rc != PGM_OK) error("pgm_kmer_cosine failed (%d): %s", rc, pgm_last_error());
    }
    void kmer_cosine_multi(uint32_t nfam, const uint32_t *nseq, uint32_t ncols, const int32_t *counts, double *cosine, int worker) override {
        int rc = pgm_kmer_cosine_multi(ctx_of(worker), nfam, nseq, ncols, counts, cosine);
        if (rc != PGM_OK) error("pgm_kmer_cosine_multi failed (%d): %s", rc, pgm_last_error());
    }
    bool prealigned_counts_multi(uint32_t dim, uint32_t nfam, const uint32_t *nrows, const uint32_t *ncols, const int8_t *rows, uint32_t npairs,
                                 const uint32_t *fam, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) override {
        int rc = pgm_prealigned_counts_multi(ctx_of(worker), dim, nfam, nrows, ncols, rows, npairs, fam, pi, pj, counts, gaps);
        if (rc != PGM_OK) error("pgm_prealigned_counts_multi failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    bool prealigned_counts_resampled(uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t nrep, const uint32_t *cols, uint32_t npairs,
                                     const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) override {
        int rc = pgm_prealigned_counts_resampled(ctx_of(worker), dim, nrows, ncols, rows, nrep, cols, npairs, pi, pj, counts, gaps);
        if (rc != PGM_OK) error("pgm_prealigned_counts_resampled failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    void msa_agreement(uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where, uint32_t *res_hits, uint32_t *pair_hits, int worker) override {
        int rc = pgm_msa_agreement(ctx_of(worker), nrows, ncols, nrep, where, res_hits, pair_hits);
        if (rc != PGM_OK) error("pgm_msa_agreement failed (%d): %s", rc, pgm_last_error());
    }
    void transfer_min(uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi,
                      int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_transfer_min(c, nleaves, nref, ref, nrep, rep_off, rep, phi);
        if (rc != PGM_OK) error("pgm_transfer_min failed (%d): %s", rc, pgm_last_error());
        transfer_stats.kernel_ms += pgm_transfer_last_kernel_ms(c);
    }
    void transfer_taxa(uint32_t nleaves, uint32_t nref, const uint64_t *ref, const uint32_t *thr, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep,
                       uint32_t *phi, uint32_t *arg, uint32_t *moved, uint32_t *counted, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_transfer_taxa(c, nleaves, nref, ref, thr, nrep, rep_off, rep, phi, arg, moved, counted);
        if (rc != PGM_OK) error("pgm_transfer_taxa failed (%d): %s", rc, pgm_last_error());
        taxa_stats.kernel_ms += pgm_transfer_last_kernel_ms(c);
    }
    void tree_likelihood(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                         const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_likelihood(c, dim, nleaves, nnodes, parent, ncols, rows, pi, P, derivs, site_l, site_k, d1, d2);
        if (rc != PGM_OK) error("pgm_tree_likelihood failed (%d): %s", rc, pgm_last_error());
        ml_tree_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_likelihood_rates(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                               uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post, double *d1, double *d2,
                               int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_likelihood_rates(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, derivs, site_l, site_k, post, d1, d2);
        if (rc != PGM_OK) error("pgm_tree_likelihood_rates failed (%d): %s", rc, pgm_last_error());
        ml_tree_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_ancestral(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                        const double *w, const double *P, double *site_l, int32_t *site_k, double *post, int8_t *anc_state, double *anc_prob, double *anc_post,
                        int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_ancestral(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, site_l, site_k, post, anc_state, anc_prob, anc_post);
        if (rc != PGM_OK) error("pgm_tree_ancestral failed (%d): %s", rc, pgm_last_error());
        ml_tree_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_ancestral_joint(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                              const double *w, const double *P, double *site_l, int32_t *site_k, double *post, uint8_t *cat, int8_t *joint_state, double *joint_l,
                              int32_t *joint_k, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_ancestral_joint(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, site_l, site_k, post, cat, joint_state, joint_l, joint_k);
        if (rc != PGM_OK) error("pgm_tree_ancestral_joint failed (%d): %s", rc, pgm_last_error());
        ml_tree_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_ancestral_sample(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                               const double *w, const double *P, uint32_t nsamp, uint64_t first_sample, uint64_t seed, double *site_l, int32_t *site_k, double *post,
                               uint8_t *samp_cat, int8_t *samp_state, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_ancestral_sample(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, nsamp, first_sample, seed, site_l, site_k, post, samp_cat, samp_state);
        if (rc != PGM_OK) error("pgm_tree_ancestral_sample failed (%d): %s", rc, pgm_last_error());
        ml_tree_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_nni(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                  const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, double *site_l, int32_t *site_k,
                  double *post, double *rho, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_nni(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cand_v, cand_a, cand_c, site_l, site_k, post, rho);
        if (rc != PGM_OK) error("pgm_tree_nni failed (%d): %s", rc, pgm_last_error());
        ml_search_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_nni_edge(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                       const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, const double *Pc,
                       double *site_l, int32_t *site_k, double *post, double *rho, double *d1, double *d2, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_nni_edge(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cand_v, cand_a, cand_c, Pc, site_l, site_k, post, rho, d1, d2);
        if (rc != PGM_OK) error("pgm_tree_nni_edge failed (%d): %s", rc, pgm_last_error());
        ml_nni_opt_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void tree_spr(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                  const double *w, const double *P, const double *Ph, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_y, double *site_l, int32_t *site_k,
                  double *post, double *rho, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_tree_spr(c, dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, Ph, ncand, cand_v, cand_y, site_l, site_k, post, rho);
        if (rc != PGM_OK) error("pgm_tree_spr failed (%d): %s", rc, pgm_last_error());
        ml_spr_stats.kernel_ms += pgm_treelik_last_kernel_ms(c);
    }
    void resampled_sums(uint32_t nrow, uint32_t ncols, const double *x, uint32_t nrep, const uint32_t *cols, double *out, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_resampled_sums(c, nrow, ncols, x, nrep, cols, out);
        if (rc != PGM_OK) error("pgm_resampled_sums failed (%d): %s", rc, pgm_last_error());
        ml_support_stats.kernel_ms += pgm_resample_last_kernel_ms(c);
    }
    bool bionj_multi(uint32_t nfam, const uint32_t *n, const double *D, const double *V, pgm_bionj_join *joins, double *final_d, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_bionj_multi(c, nfam, n, D, V, joins, final_d);
        if (rc != PGM_OK) error("pgm_bionj_multi failed (%d): %s", rc, pgm_last_error());
        ++bionj_device_calls;
        bionj_launches += pgm_bionj_last_launches(c);
        return true;
    }
    bool bionj_plan_multi(uint32_t nfam, const uint32_t *n, const double *D, const double *V, const pgm_bionj_pair *plan, pgm_bionj_join *joins, double *final_d,
                          int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_bionj_plan_multi(c, nfam, n, D, V, plan, joins, final_d);
        if (rc != PGM_OK) error("pgm_bionj_plan_multi failed (%d): %s", rc, pgm_last_error());
        ++bionj_device_calls;
        bionj_launches += pgm_bionj_last_launches(c);
        return true;
    }
    bool gapmask_extend_batch(uint32_t njobs, const pgm_gapmask_job *jobs, int worker) override {
        int rc = pgm_gapmask_extend_batch(ctx_of(worker), njobs, jobs);
        if (rc != PGM_OK) error("pgm_gapmask_extend_batch failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    void wls_load(uint32_t n, const double *D, const double *W, int worker) override {
        int rc = pgm_wls_load(ctx_of(worker), n, D, W);
        if (rc != PGM_OK) error("pgm_wls_load failed (%d): %s", rc, pgm_last_error());
    }
    void wls_pair_sums_batch(uint32_t njobs, const pgm_wls_job *jobs, double *out, int worker) override {
        pgm_ctx *c = ctx_of(worker);
        int rc = pgm_wls_pair_sums_batch(c, njobs, jobs, out);
        if (rc != PGM_OK) error("pgm_wls_pair_sums_batch failed (%d): %s", rc, pgm_last_error());
        seconds_wls_kernels += pgm_wls_last_kernel_ms(c) * 1e-3;
        wls_launches += pgm_wls_last_launches(c);
    }
    bool gap_parsimony_batch(uint32_t njobs, const pgm_parsimony_job *jobs, uint32_t *scores, int worker) override {
        int rc = pgm_gap_parsimony_batch(ctx_of(worker), njobs, jobs, scores);
        if (rc != PGM_OK) error("pgm_gap_parsimony_batch failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    bool merge_profiles_batch(uint32_t njobs, const pgm_merge_job *jobs, int worker) override {
        int rc = pgm_merge_profiles_batch(ctx_of(worker), njobs, jobs);
        if (rc != PGM_OK) error("pgm_merge_profiles_batch failed (%d): %s", rc, pgm_last_error());
        return true;
    }
    void csprofile_create_batch(const CSProfile &lib, uint32_t nseq, const int8_t *syms, const uint32_t *offs,
                                const double *tau, const double *pi, const double *p_uniform, double *out,
                                const uint64_t *out_offs, int worker) override {
        pgm_ctx *ctx = ctx_of(worker);
        const size_t slot = (size_t)worker % ctxs.size();
        if (loaded[slot] != &lib) {
            int rc = pgm_csprofile_load(ctx, (uint32_t)lib.nprof(), (uint32_t)lib.ncols(), lib.lprofiles().data(),
                                        lib.centre().data(), lib.priors().data());
            if (rc != PGM_OK) error("pgm_csprofile_load failed (%d): %s", rc, pgm_last_error());
            loaded[slot] = &lib;
        }
        int rc = pgm_csprofile_create_batch(ctx, nseq, syms, offs, tau, pi, p_uniform, out, out_offs);
        if (rc != PGM_OK) error("pgm_csprofile_create_batch failed (%d): %s", rc, pgm_last_error());
    }
    void csprofile_preload(const CSProfile &lib) override {
        for (size_t slot = 0; slot < ctxs.size(); ++slot) {
            if (loaded[slot] == &lib) continue;
            int rc = pgm_csprofile_load(ctxs[slot], (uint32_t)lib.nprof(), (uint32_t)lib.ncols(), lib.lprofiles().data(), lib.centre().data(), lib.priors().data());
            if (rc != PGM_OK) error("pgm_csprofile_load failed (%d): %s", rc, pgm_last_error());
            loaded[slot] = &lib;
        }
    }
    bool csprofile_create_batch_res(const CSProfile &lib, uint32_t nseq, const int8_t *syms, const uint32_t *offs, const double *tau, const double *pi,
                                    const double *p_uniform, const double **dev, int worker) override {
        pgm_ctx *ctx = ctx_of(worker);
        const size_t slot = (size_t)worker % ctxs.size();
        if (loaded[slot] != &lib) {
            int rc = pgm_csprofile_load(ctx, (uint32_t)lib.nprof(), (uint32_t)lib.ncols(), lib.lprofiles().data(), lib.centre().data(), lib.priors().data());
            if (rc != PGM_OK) error("pgm_csprofile_load failed (%d): %s", rc, pgm_last_error());
            loaded[slot] = &lib;
        }
        int rc = pgm_csprofile_create_batch_res(ctx, nseq, syms, offs, tau, pi, p_uniform, dev);
        if (rc != PGM_OK) error("pgm_csprofile_create_batch_res failed (%d): %s", rc, pgm_last_error());
        return true;
    }
};
}  // namespace

Backend &default_backend() {
    static HipBackend be;
    return be;
}
}  // namespace pgm
