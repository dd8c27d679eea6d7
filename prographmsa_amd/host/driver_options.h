// driver_options.h — what the command line asks of the driver itself (main.cpp and the driver_*.cpp files).  What the whole host
// reads stays in cmdlineopts (pgm_host.h); parse_driver_options fills both.
#pragma once
#include "pgm_host.h"

namespace pgm {

struct BootstrapOpts {   // --bootstrap N --bootstrap_out FILE --bootstrap_seed S
    bool given = false, out_given = false;
    long long n = 0;
    std::string out, tbe, trees;   // --bootstrap_tbe FILE, --bootstrap_trees FILE
    std::string taxa, taxa_edges;   // --bootstrap_taxa FILE, --bootstrap_taxa_edges FILE
    bool cutoff_given = false;   // --bootstrap_taxa_cutoff X
    double cutoff = 0.3;
    uint64_t seed = 1;
    bool any_taxa() const { return !taxa.empty() || !taxa_edges.empty() || cutoff_given; }
    bool any() const { return given || out_given || !tbe.empty() || !trees.empty() || any_taxa(); }
};

struct GuidanceOpts {   // --guidance N --guidance_out FILE --guidance_seed S --guidance_residues FILE --guidance_dump PREFIX
    bool given = false, out_given = false;
    long long n = 0;
    std::string out, residues, dump;
    uint64_t seed = 1;
    bool any() const { return given || out_given || !residues.empty() || !dump.empty(); }
};

struct MlTreeOpts {   // --ml_tree FILE --ml_sites FILE --ml_rounds N --ml_epsilon X --ml_gamma K --ml_alpha X --ml_rates FILE
                      // --ml_ancestral FILE --ml_ancestral_tree FILE --ml_ancestral_probs FILE --ml_search N --ml_start FILE --ml_search_log FILE
                      // --ml_support FILE --ml_support_table FILE --ml_support_reps N --ml_support_seed S --ml_nni_opt N --ml_spr R
                      // --ml_ancestral_joint FILE --ml_ancestral_joint_sites FILE --ml_ancestral_samples N --ml_ancestral_samples_out FILE
                      // --ml_ancestral_samples_seed S
    std::string tree, sites, rates, anc, anc_tree, anc_probs;
    bool anc_given = false, anc_tree_given = false, anc_probs_given = false;
    bool any_anc() const { return anc_given || anc_tree_given || anc_probs_given; }
    // --ml_ancestral_joint, --ml_ancestral_samples: the jointly most probable states; N draws from the posterior
    std::string joint, joint_sites, samples_out;
    bool joint_given = false, joint_sites_given = false, samples_given = false, samples_out_given = false, samples_seed_given = false;
    long samples = 0;
    uint64_t samples_seed = 1;
    bool any_joint() const { return joint_given || joint_sites_given || samples_given || samples_out_given || samples_seed_given; }
    bool tree_given = false, sites_given = false, rounds_given = false, eps_given = false, gamma_given = false, alpha_given = false, rates_given = false;
    long rounds = 100, gamma = 0;
    double eps = 1e-4, alpha = 1.0;
    bool search_given = false, start_given = false, search_log_given = false;
    long search = 0;
    std::string start, search_log;
    std::shared_ptr<PhyTree> start_tree;   // --ml_start as read and checked against the family's names, before any work (main.cpp)
    bool nni_opt_given = false;   // --ml_nni_opt N: the Newton rounds on the central branch of every interchange
    long nni_opt = 0;
    bool spr_given = false;   // --ml_spr R: an SPR scan of radius R where the interchanges of the search stall
    long spr = 0;
    bool any_search() const { return search_given || start_given || search_log_given; }
    bool support_given = false, support_table_given = false, support_reps_given = false, support_seed_given = false;
    std::string support, support_table;
    long support_reps = 1000;
    uint64_t support_seed = 1;
    bool any_support() const { return support_given || support_table_given || support_reps_given || support_seed_given; }
    bool any() const {
        return tree_given || sites_given || rounds_given || eps_given || gamma_given || alpha_given || rates_given || any_anc() || any_search() || any_support() || nni_opt_given || spr_given || any_joint();
    }
};

struct DriverOptions {
    BootstrapOpts bootstrap;
    GuidanceOpts guidance;
    MlTreeOpts mltree;
    bool iters_set = false, stats = false;
    bool indel_set = false, edgehl_set = false, maxdist_set = false, cutdist_set = false;   // (the defaults --codon rescales)
    std::string dump, dist_dump, joins_dump;   // --dump_jobs, --dump_dist, --dump_joins
    std::string batch_list, topo_file;   // --batch, --topology
    double batch_cells = 2e9;   // --batch_cells: estimated DP cells of one chunk of families, of one group of --guidance replicates
};

void usage();
// The command line into cmdlineopts and `o`.  Returns -1 to go on, or the exit code of a command line that ends the run here: the
// usage text or the message is then written.
int parse_driver_options(int argc, char **argv, DriverOptions &o);

}  // namespace pgm
