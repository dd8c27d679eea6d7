// driver_stats.cpp — the --stats line: one JSON record on stderr; the groups of keys of an option only when the option was given.
#include "driver.h"

#include <cstdio>

namespace pgm {

void print_stats(const DriverOptions &o, double t_init, double t_tree, double t_prog, bool batch) {
    Backend &be = default_backend();
    fprintf(stderr,
            "{\"backend\": \"%s\", \"init_s\": %.6f, \"tree_s\": %.6f, \"progressive_s\": %.6f, \"align_cells\": %llu, \"align_s\": %.6f, "
            "\"nw_cells\": %llu, \"nw_s\": %.6f, \"mldist_s\": %.6f, \"merge_profiles_s\": %.6f, \"farm_workers\": %d, \"farm_tiles\": %d, \"farm_level_workers\": %d, \"farm_leaf_workers\": %d, \"resident\": %s, \"resident_imports\": %d, \"bionj_s\": %.6f, \"bionj_device_calls\": %llu, \"bionj_launches\": %llu, \"switches\": \"%s\"",
            be.name(), t_init, t_tree, t_prog, (unsigned long long)be.cells_aligned, be.seconds_align,
            (unsigned long long)be.cells_nw, be.seconds_nw, be.seconds_mldist, be.seconds_merge_profiles, be.farm_workers, be.farm_tiles, be.farm_level_workers, be.farm_leaf_workers, be.resident_pass ? "true" : "false", be.resident_imports,
            be.seconds_bionj, (unsigned long long)be.bionj_device_calls, (unsigned long long)be.bionj_launches, host_switches().describe().c_str());
    if (cmdlineopts.reroot_flag) {   // (keys of the root search only when it ran)
        const RootSearchStats &r = root_search_stats;
        fprintf(stderr, ", \"reroot\": %d, \"reroot_merges\": %d, \"reroot_candidates\": %d, \"reroot_heights\": %d, \"reroot_batches\": %d, "
                        "\"reroot_align_s\": %.6f, \"reroot_host_merge_s\": %.6f, \"reroot_gapmask_s\": %.6f, \"reroot_parsimony_s\": %.6f, \"reroot_rows_s\": %.6f",
                cmdlineopts.reroot_flag, r.merges, r.candidates, r.heights, r.batches, r.align_s, r.host_merge_s, r.gapmask_s, r.parsimony_s, r.select_s);
    }
    if (cmdlineopts.wlsrefine_flag) {   // (keys of the refinement only when it ran)
        const WlsStats &w = wls_stats;
        fprintf(stderr, ", \"wls_refine\": %d, \"wls_trees\": %d, \"wls_s\": %.6f, \"wls_pair_sums_s\": %.6f, \"wls_kernels_s\": %.6f, \"wls_sweeps\": %d, "
                        "\"wls_quartets\": %llu, \"wls_quintets\": %llu, \"wls_batches\": %llu, \"wls_launches\": %llu",
                cmdlineopts.wlsrefine_flag, w.trees, w.seconds, w.pair_sums_s, be.seconds_wls_kernels, w.sweeps, (unsigned long long)w.quartets,
                (unsigned long long)w.quintets, (unsigned long long)w.batches, (unsigned long long)be.wls_launches);
    }
    if (host_switches().device_mldist)   // (keys of PGM_DEVICE_MLDIST only: pairs estimated by the device kernel, its time)
        fprintf(stderr, ", \"mldist_device_pairs\": %llu, \"mldist_kernel_ms\": %.3f", (unsigned long long)be.mldist_device_pairs, be.mldist_kernel_ms);
    if (o.bootstrap.given)   // (keys of --bootstrap only)
        fprintf(stderr, ", \"bootstrap_replicates\": %d, \"bootstrap_s\": %.6f, \"bootstrap_counts_calls\": %llu", bootstrap_stats.replicates, bootstrap_stats.seconds,
                (unsigned long long)bootstrap_stats.counts_calls);
    if (!o.bootstrap.tbe.empty())   // (keys of --bootstrap_tbe only)
        fprintf(stderr, ", \"bootstrap_tbe_s\": %.6f, \"bootstrap_transfer_calls\": %llu, \"bootstrap_transfer_kernel_ms\": %.3f", transfer_stats.seconds,
                (unsigned long long)transfer_stats.calls, transfer_stats.kernel_ms);
    if (!o.bootstrap.taxa.empty())   // (keys of --bootstrap_taxa only)
        fprintf(stderr, ", \"bootstrap_taxa_s\": %.6f, \"bootstrap_taxa_calls\": %llu, \"bootstrap_taxa_kernel_ms\": %.3f", taxa_stats.seconds,
                (unsigned long long)taxa_stats.calls, taxa_stats.kernel_ms);
    if (o.guidance.given)   // (keys of --guidance only)
        fprintf(stderr, ", \"guidance_replicates\": %d, \"guidance_s\": %.6f, \"guidance_align_s\": %.6f, \"guidance_agreement_s\": %.6f, "
                        "\"guidance_passes\": %llu, \"guidance_agreement_calls\": %llu",
                guidance_stats.replicates, guidance_stats.seconds, guidance_stats.align_s, guidance_stats.agreement_s, (unsigned long long)guidance_stats.passes,
                (unsigned long long)guidance_stats.agreement_calls);
    if (o.mltree.tree_given)   // (keys of --ml_tree only)
        fprintf(stderr, ", \"ml_tree_s\": %.6f, \"ml_rounds\": %llu, \"ml_evaluations\": %llu, \"ml_lnl_start\": %.17g, \"ml_lnl\": %.17g, \"ml_kernel_ms\": %.3f",
                ml_tree_stats.seconds, (unsigned long long)ml_tree_stats.rounds, (unsigned long long)ml_tree_stats.evaluations, ml_tree_stats.lnl_start, ml_tree_stats.lnl,
                ml_tree_stats.kernel_ms);
    if (o.mltree.gamma_given)   // (keys of --ml_gamma only)
        fprintf(stderr, ", \"ml_categories\": %u, \"ml_alpha\": %.17g", ml_tree_stats.categories, ml_tree_stats.alpha);
    if (o.mltree.anc_given)   // (key of --ml_ancestral only)
        fprintf(stderr, ", \"ml_ancestral_s\": %.6f", ml_tree_stats.ancestral_s);
    if (o.mltree.joint_given)   // (key of --ml_ancestral_joint only)
        fprintf(stderr, ", \"ml_ancestral_joint_s\": %.6f", ml_tree_stats.ancestral_joint_s);
    if (o.mltree.samples_given)   // (key of --ml_ancestral_samples only)
        fprintf(stderr, ", \"ml_ancestral_samples_s\": %.6f", ml_tree_stats.ancestral_samples_s);
    if (o.mltree.search_given)   // (keys of --ml_search only)
        fprintf(stderr, ", \"ml_search_s\": %.6f, \"ml_search_rounds\": %llu, \"ml_nni_applied\": %llu, \"ml_nni_calls\": %llu, \"ml_nni_kernel_ms\": %.3f",
                ml_search_stats.seconds, (unsigned long long)ml_search_stats.rounds, (unsigned long long)ml_search_stats.applied,
                (unsigned long long)ml_search_stats.calls, ml_search_stats.kernel_ms);
    if (o.mltree.support_given)   // (keys of --ml_support only)
        fprintf(stderr, ", \"ml_support_s\": %.6f, \"ml_support_nodes\": %llu, \"ml_support_calls\": %llu, \"ml_support_kernel_ms\": %.3f", ml_support_stats.seconds,
                (unsigned long long)ml_support_stats.nodes, (unsigned long long)ml_support_stats.calls, ml_support_stats.kernel_ms);
    if (o.mltree.nni_opt_given)   // (keys of --ml_nni_opt only)
        fprintf(stderr, ", \"ml_nni_opt_s\": %.6f, \"ml_nni_opt_calls\": %llu, \"ml_nni_opt_kernel_ms\": %.3f", ml_nni_opt_stats.seconds,
                (unsigned long long)ml_nni_opt_stats.calls, ml_nni_opt_stats.kernel_ms);
    if (o.mltree.spr_given)   // (keys of --ml_spr only)
        fprintf(stderr, ", \"ml_spr_s\": %.6f, \"ml_spr_calls\": %llu, \"ml_spr_candidates\": %llu, \"ml_spr_applied\": %llu, \"ml_spr_kernel_ms\": %.3f",
                ml_spr_stats.seconds, (unsigned long long)ml_spr_stats.calls, (unsigned long long)ml_spr_stats.candidates, (unsigned long long)ml_spr_stats.applied,
                ml_spr_stats.kernel_ms);
    if (batch)   // (keys of --batch only)
        fprintf(stderr, ", \"batch_families\": %d, \"batch_failed\": %d, \"batch_chunks\": %d, \"batch_passes\": %llu, \"batch_levels\": %llu, "
                        "\"batch_align_calls\": %llu, \"batch_dist_calls\": %llu",
                batch_stats.families, batch_stats.failed, batch_stats.chunks, (unsigned long long)batch_stats.passes, (unsigned long long)batch_stats.levels,
                (unsigned long long)be.calls_align.load(), (unsigned long long)be.calls_dist.load());
    fprintf(stderr, "}\n");
}

}  // namespace pgm
