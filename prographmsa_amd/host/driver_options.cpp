// driver_options.cpp — the driver's command line: the usage text, the flags (TCLAP is not available, so a minimal parser accepts
// the reference's spellings) and what is refused before anything is read.
#include "driver_options.h"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <iostream>

namespace pgm {

// (tests/test_cpu_driver.py pins this text by its checksum: --ml_ancestral, --ml_ancestral_tree and --ml_ancestral_probs, which came
// after that, are described in README.md and DESIGN.md 3.19)
void usage() {
    std::cerr << "USAGE: pgmsa [-f|--fasta] [-t|--tree <newick>] [--topology <newick>] [-o <file>] [-T] [-I] [-a] [-m] [-M]\n"
                 "             [--codon] [-c|--cs_profile <lib>] [-i <iters>] [-g rate] [-e prob] [-E prob]\n"
                 "             [-s prob] [-A] [--early_refinement] [--ancestral_seqs] [--profile_out <file>] [-R] [--read_repeats <file>]\n"
                 "             [-r|--reroot [-r]] [-W|--wls_refine [-W]] [--dna] [--custom_model <file>] [-F|--estimate_aafreqs]\n"
                 "             [-C|--aafreqs_pseudocount <count>] [--dump_jobs <file>] [--dump_dist <file>] [--dump_joins <file>] [--stats]\n"
                 "             [--bootstrap <N> --bootstrap_out <file> [--bootstrap_seed <S>] [--bootstrap_tbe <file>] [--bootstrap_trees <file>]\n"
                 "              [--bootstrap_taxa <file> [--bootstrap_taxa_cutoff <X>] [--bootstrap_taxa_edges <file>]]]\n"
                 "             [--guidance <N> --guidance_out <file> [--guidance_seed <S>] [--guidance_residues <file>] [--guidance_dump <prefix>]]\n"
                 "             [--ml_tree <file> [--ml_sites <file>] [--ml_rounds <N>] [--ml_epsilon <X>]\n"
                 "              [--ml_gamma <K> [--ml_alpha <X>] [--ml_rates <file>]]]\n"
                 "             <fasta file>\n"
                 "       pgmsa --batch <list> [--batch_cells <cells>] [options]\n"
                 "  --batch <list>  align many families in one run: every line of <list> is input.fa<TAB>output[<TAB>guide_tree.nwk[<TAB>topology.nwk]]\n"
                 "                (an empty third field: no guide tree; blank lines and lines starting with # are skipped); the other options\n"
                 "                apply to every family and every output is what the same options write for that family alone.  Not with a\n"
                 "                positional file, -o, -t, --topology, -r, -W, -R, --read_repeats, --profile_out, --dump_jobs, --dump_dist,\n"
                 "                --dump_joins\n"
                 "  --topology <newick>  every guide tree the run estimates (the initial one unless -t is given, and the one after every\n"
                 "                pass) keeps the topology of this tree; only its branch lengths are estimated.  The file needs a branch\n"
                 "                length on every edge (the values are ignored) and two children at every node; every sequence must be a\n"
                 "                leaf, leaves that are no sequence are pruned\n"
                 "  --batch_cells <cells>  families share the device stages in chunks of at most this many estimated DP cells per pass\n"
                 "                (default 2e9); a larger family is a chunk of its own\n"
                 "  --dna         align DNA sequences (T C A G; U reads as T; N, X and the IUPAC ambiguity codes as unknown); needs\n"
                 "                --custom_model\n"
                 "  --custom_model <file>  custom substitution model: the strict lower triangle of the symmetric exchangeability\n"
                 "                matrix row by row (rows 1 .. D-1, columns below the diagonal), then the D equilibrium frequencies,\n"
                 "                separated by white space, in the alphabet's own order: TCAG for --dna, ACDEFGHIKLMNPQRSTVWY for amino\n"
                 "                acids (alphabetical by one-letter code, not PAML's ARNDCQEGHILKMFPSTWYV), the 61 sense codons in TCAG\n"
                 "                order for --codon\n"
                 "  -F, --estimate_aafreqs  estimate the equilibrium frequencies from the input sequences\n"
                 "  -C, --aafreqs_pseudocount <count>  pseudo-count of the model's own frequencies in that estimate (default 1000)\n"
                 "  -m, -M        maximum-likelihood distances (-M: with the gap term).  The host estimates them unless the environment\n"
                 "                sets PGM_DEVICE_MLDIST=1; the device then estimates them where the backend has the kernel: a model\n"
                 "                with an eigen form of up to 20 states, and, on the GPU backend, any model of up to 64 states, --codon\n"
                 "                and a model without an eigen form included (last-bit differences to the host's values)\n"
                 "  -r, --reroot  realign with the guide tree rooted on every branch and keep the alignment of the lowest gap\n"
                 "                parsimony score; given twice (-rr), a hill climb over neighbouring branches instead\n"
                 "  --bootstrap <N>  bootstrap support (1 <= N <= 1000) for the tree estimated from the final alignment (the tree -T prints\n"
                 "                after a further round): N resamplings of the alignment's columns, a BioNJ tree of each, and for every internal\n"
                 "                edge the number of replicate trees with the same split of the sequences.  --bootstrap_out <file> (required)\n"
                 "                gets that tree with the counts as node labels; --bootstrap_seed <S> (default 1) seeds the resampling.  Needs\n"
                 "                at least 4 sequences; not with --batch, -W, -r, --topology\n"
                 "  --bootstrap_tbe <file>  with --bootstrap: the same tree with the transfer bootstrap expectation (TBE, Lemoine et al. 2018) of\n"
                 "                every internal edge as node labels (%.6f): 1 - the mean over the replicates of the fewest leaves to move for the\n"
                 "                replicate to have the edge, over the size of the edge's smaller side - 1\n"
                 "  --bootstrap_trees <file>  with --bootstrap: the N replicate trees, one newick line each, in replicate order\n"
                 "  --bootstrap_taxa <file>  with --bootstrap: per sequence how often it is among the fewest leaves to move for a replicate to\n"
                 "                have an edge (the taxon side of the transfer bootstrap: unstable, \"rogue\" sequences score high).  Counted are\n"
                 "                the (edge, replicate) pairs whose transfer index is at most X times the size of the edge's smaller side - 1,\n"
                 "                --bootstrap_taxa_cutoff <X> (0 <= X < 1, default 0.3); among equally near replicate edges the first in sorted\n"
                 "                order is taken.  One line per sequence in sorted-name order: name, times moved, that over the counted pairs.\n"
                 "                --bootstrap_taxa_edges <file>: the same counts per labelled node of the --bootstrap_out tree\n"
                 "  --guidance <N>  confidence of the alignment under perturbed guide trees (1 <= N <= 1000): the BioNJ trees of N resamplings of\n"
                 "                the final alignment's columns (those of --bootstrap for the same N and seed), midpoint rooted, are each used as\n"
                 "                the guide tree of a realignment, and every residue pair, column and sequence of the alignment written is scored\n"
                 "                by how often the replicate alignments put the same residues in one column.  --guidance_out <file> (required)\n"
                 "                gets the alignment, column, sequence and sequence-pair lines (tab separated: hits, pairs, hits / pairs);\n"
                 "                --guidance_residues <file> a line per residue; --guidance_seed <S> (default 1) seeds the resampling;\n"
                 "                --guidance_dump <prefix> writes every replicate's guide tree and alignment to <prefix>.<r>.nwk / .fa.  The\n"
                 "                replicates share the device stages in groups of at most --batch_cells estimated DP cells.  Needs at least 4\n"
                 "                sequences; not with --batch, -T, -r, -W, --topology\n"
                 "  --ml_tree <file>  maximum-likelihood branch lengths for the tree estimated from the final alignment (the tree of --bootstrap):\n"
                 "                the likelihood of the alignment as written under the run's substitution model, gaps and residues without a\n"
                 "                value as missing data, is maximised over the branch lengths (each within 1e-6 .. 10) on the fixed topology and\n"
                 "                root; <file> gets the tree with those lengths.  --ml_sites <file>: a line `lnL <value>`, then the\n"
                 "                log-likelihood of every column (column<TAB>value, columns from 1).  --ml_rounds <N> (1 <= N <= 10000, default\n"
                 "                100) bounds the rounds of the optimiser, --ml_epsilon <X> (X >= 0, default 1e-4) is the gain of lnL below\n"
                 "                which it stops.  Needs at least 3 sequences; not with --batch, -W, -r, --topology\n"
                 "  --ml_gamma <K>  with --ml_tree: rate variation across columns by a discrete gamma of <K> (2 .. 16) equally probable\n"
                 "                categories of mean 1; the likelihood and --ml_sites are the mixture's.  --ml_alpha <X> (0.05 <= X <= 100)\n"
                 "                fixes the shape; without it the shape is estimated together with the branch lengths (--ml_rounds then bounds\n"
                 "                every run of the branch-length loop).  --ml_rates <file>: `alpha<TAB>value`, per category\n"
                 "                `rate<TAB>k<TAB>value`, then per column `column<TAB>posterior mean rate<TAB>most probable category`\n"
                 "  -W, --wls_refine  refine every guide tree estimated from distances by weighted least squares (nearest-neighbour\n"
                 "                interchanges of quartets); given twice (-WW), quintet moves as well\n";
}

// (--ml_ancestral_joint, --ml_ancestral_joint_sites, --ml_ancestral_samples, --ml_ancestral_samples_out and
// --ml_ancestral_samples_seed came later still: README.md and DESIGN.md 3.24)
// "the whole text is a number": not empty and nothing after the number.  The ranges differ and stay with the callers.
static bool whole_number(const std::string &text, long &v) {
    char *end = nullptr;
    v = strtol(text.c_str(), &end, 10);
    return !text.empty() && *end == '\0';
}
// a seed: decimal digits alone, within 64 bits
static bool whole_seed(const std::string &text, uint64_t &v) {
    if (text.empty() || text.find_first_not_of("0123456789") != std::string::npos) return false;
    errno = 0;
    v = strtoull(text.c_str(), nullptr, 10);
    return errno == 0;
}
static bool real_number(const std::string &text, double &v) {
    char *end = nullptr;
    v = strtod(text.c_str(), &end);
    return !text.empty() && *end == '\0';
}

int parse_driver_options(int argc, char **argv, DriverOptions &o) {
    bool missing = false;   // a flag without its value
    bool cutoff_ok = true, rounds_ok = true, eps_ok = true, gamma_ok = true, alpha_ok = true, search_ok = true, reps_ok = true, nni_opt_ok = true, spr_ok = true, samples_ok = true, samples_seed_ok = true;
    for (int i = 1; i < argc && !missing; ++i) {
        std::string s = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { missing = true; return ""; } return argv[++i]; };
        if (s == "-f" || s == "--fasta") cmdlineopts.fasta_flag = true;
        else if (s == "-t" || s == "--tree") cmdlineopts.tree_file = val();
        else if (s == "--topology") o.topo_file = val();
        else if (s == "-o" || s == "--output") cmdlineopts.output_file = val();
        else if (s == "-T" || s == "--only_tree") cmdlineopts.onlytree_flag = true;
        else if (s == "-I" || s == "--input_order") cmdlineopts.inputorder_flag = true;
        else if (s == "-a" || s == "--nwdist") cmdlineopts.nwdist_flag = true;
        else if (s == "-m" || s == "--mldist") cmdlineopts.mldist_flag = true;
        else if (s == "-M" || s == "--mldist_gap") cmdlineopts.mldist_gap_flag = true;
        else if (s == "-A" || s == "--no_force_align") cmdlineopts.noforcealign_flag = true;
        else if (s == "--codon") cmdlineopts.codon_flag = true;
        else if (s == "--dna") cmdlineopts.dna_flag = true;
        else if (s == "--custom_model") cmdlineopts.cmodel_file = val();
        else if (s == "-F" || s == "--estimate_aafreqs") cmdlineopts.aafreqs_flag = true;
        else if (s == "-C" || s == "--aafreqs_pseudocount") cmdlineopts.pseudo_count = atof(val().c_str());
        else if (s == "-c" || s == "--cs_profile") cmdlineopts.cs_file = val();
        else if (s == "-i" || s == "--iterations") { cmdlineopts.iters = atoi(val().c_str()); o.iters_set = true; }
        else if (s == "-g" || s == "--indel_rate") { cmdlineopts.indel_rate = atof(val().c_str()); o.indel_set = true; }
        else if (s == "-e" || s == "--gap_ext") cmdlineopts.gapext_prob = atof(val().c_str());
        else if (s == "-E" || s == "--end_indel_prob") cmdlineopts.end_indel_prob = atof(val().c_str());
        else if (s == "-s" || s == "--altsplice_prob") cmdlineopts.altsplice_prob = atof(val().c_str());
        else if (s == "-l" || s == "--edge_halflife") { cmdlineopts.edge_halflife = atof(val().c_str()); o.edgehl_set = true; }
        else if (s == "-x" || s == "--cutoff_dist") { cmdlineopts.cutoff_dist = atof(val().c_str()); o.cutdist_set = true; }
        else if (s == "-d" || s == "--min_dist") cmdlineopts.min_dist = atof(val().c_str());
        else if (s == "-D" || s == "--max_dist") { cmdlineopts.max_dist = atof(val().c_str()); o.maxdist_set = true; }
        else if (s == "-p" || s == "--min_pdist") cmdlineopts.min_pdist = atof(val().c_str());
        else if (s == "-P" || s == "--max_pdist") cmdlineopts.max_pdist = atof(val().c_str());
        else if (s == "--ancestral_seqs") cmdlineopts.ancestral_flag = true;
        else if (s == "--early_refinement") cmdlineopts.earlyref_flag = true;
        else if (s == "--profile_out") cmdlineopts.profile_file = val();
        else if (s == "--read_repeats") cmdlineopts.readreps_file = val();
        else if (s == "-R" || s == "--repeats") cmdlineopts.repeats_flag = true;
        else if (s == "--dump_jobs") o.dump = val();
        else if (s == "--dump_dist") o.dist_dump = val();
        else if (s == "--dump_joins") o.joins_dump = val();
        else if (s == "--stats") o.stats = true;
        else if (s == "--batch") o.batch_list = val();
        else if (s == "--batch_cells") o.batch_cells = atof(val().c_str());
        else if (s == "--bootstrap") { o.bootstrap.given = true; o.bootstrap.n = atoll(val().c_str()); }
        else if (s == "--bootstrap_out") { o.bootstrap.out_given = true; o.bootstrap.out = val(); }
        else if (s == "--bootstrap_seed") o.bootstrap.seed = strtoull(val().c_str(), nullptr, 10);
        else if (s == "--bootstrap_tbe") o.bootstrap.tbe = val();
        else if (s == "--bootstrap_trees") o.bootstrap.trees = val();
        else if (s == "--bootstrap_taxa") o.bootstrap.taxa = val();
        else if (s == "--bootstrap_taxa_edges") o.bootstrap.taxa_edges = val();
        else if (s == "--bootstrap_taxa_cutoff") { o.bootstrap.cutoff_given = true; cutoff_ok = real_number(val(), o.bootstrap.cutoff); }
        else if (s == "--guidance") { o.guidance.given = true; o.guidance.n = atoll(val().c_str()); }
        else if (s == "--guidance_out") { o.guidance.out_given = true; o.guidance.out = val(); }
        else if (s == "--guidance_seed") o.guidance.seed = strtoull(val().c_str(), nullptr, 10);
        else if (s == "--guidance_residues") o.guidance.residues = val();
        else if (s == "--guidance_dump") o.guidance.dump = val();
        else if (s == "--ml_tree") { o.mltree.tree_given = true; o.mltree.tree = val(); }
        else if (s == "--ml_sites") { o.mltree.sites_given = true; o.mltree.sites = val(); }
        else if (s == "--ml_rounds") { o.mltree.rounds_given = true; rounds_ok = whole_number(val(), o.mltree.rounds); }
        else if (s == "--ml_epsilon") { o.mltree.eps_given = true; eps_ok = real_number(val(), o.mltree.eps); }
        else if (s == "--ml_gamma") { o.mltree.gamma_given = true; gamma_ok = whole_number(val(), o.mltree.gamma); }
        else if (s == "--ml_alpha") { o.mltree.alpha_given = true; alpha_ok = real_number(val(), o.mltree.alpha); }
        else if (s == "--ml_rates") { o.mltree.rates_given = true; o.mltree.rates = val(); }
        else if (s == "--ml_ancestral") { o.mltree.anc_given = true; o.mltree.anc = val(); }
        else if (s == "--ml_ancestral_tree") { o.mltree.anc_tree_given = true; o.mltree.anc_tree = val(); }
        else if (s == "--ml_ancestral_probs") { o.mltree.anc_probs_given = true; o.mltree.anc_probs = val(); }
        else if (s == "--ml_ancestral_joint") { o.mltree.joint_given = true; o.mltree.joint = val(); }
        else if (s == "--ml_ancestral_joint_sites") { o.mltree.joint_sites_given = true; o.mltree.joint_sites = val(); }
        else if (s == "--ml_ancestral_samples") { o.mltree.samples_given = true; samples_ok = whole_number(val(), o.mltree.samples); }
        else if (s == "--ml_ancestral_samples_out") { o.mltree.samples_out_given = true; o.mltree.samples_out = val(); }
        else if (s == "--ml_ancestral_samples_seed") { o.mltree.samples_seed_given = true; samples_seed_ok = whole_seed(val(), o.mltree.samples_seed); }
        else if (s == "--ml_search") { o.mltree.search_given = true; search_ok = whole_number(val(), o.mltree.search); }
        else if (s == "--ml_start") { o.mltree.start_given = true; o.mltree.start = val(); }
        else if (s == "--ml_search_log") { o.mltree.search_log_given = true; o.mltree.search_log = val(); }
        else if (s == "--ml_nni_opt") { o.mltree.nni_opt_given = true; nni_opt_ok = whole_number(val(), o.mltree.nni_opt); }
        else if (s == "--ml_spr") { o.mltree.spr_given = true; spr_ok = whole_number(val(), o.mltree.spr); }
        else if (s == "--ml_support") { o.mltree.support_given = true; o.mltree.support = val(); }
        else if (s == "--ml_support_table") { o.mltree.support_table_given = true; o.mltree.support_table = val(); }
        else if (s == "--ml_support_reps") { o.mltree.support_reps_given = true; reps_ok = whole_number(val(), o.mltree.support_reps); }
        else if (s == "--ml_support_seed") { o.mltree.support_seed_given = true; o.mltree.support_seed = strtoull(val().c_str(), nullptr, 10); }
        else if (s == "--reroot") ++cmdlineopts.reroot_flag;
        else if (s == "--wls_refine") ++cmdlineopts.wlsrefine_flag;
        else if (s.size() >= 2 && s[0] == '-' && s.find_first_not_of('W', 1) == std::string::npos) cmdlineopts.wlsrefine_flag += (int)s.size() - 1;   // -W, -WW
        else if (s.size() >= 2 && s[0] == '-' && s.find_first_not_of('r', 1) == std::string::npos) cmdlineopts.reroot_flag += (int)s.size() - 1;   // -r, -rr (TCLAP's MultiSwitchArg)
        else if (s == "-h" || s == "--help") { usage(); return 0; }
        else if (!s.empty() && s[0] == '-') { std::cerr << "Command line error: unknown flag " << s << std::endl; return 1; }
        else cmdlineopts.sequence_file = s;
    }
    if (missing) { usage(); return 1; }
    if (!o.batch_list.empty()) {   // what belongs to one family or is a search loop of its own is refused
        const char *refused = !cmdlineopts.sequence_file.empty() ? "a positional sequence file (the families come from the list)"
                              : !cmdlineopts.output_file.empty() ? "-o (every line of the list names its output)"
                              : !cmdlineopts.tree_file.empty() ? "-t (a guide tree is the third field of a family's line)"
                              : !o.topo_file.empty() ? "--topology (a topology is the fourth field of a family's line)"
                              : cmdlineopts.reroot_flag ? "-r" : cmdlineopts.wlsrefine_flag ? "-W"
                              : cmdlineopts.repeats_flag ? "-R" : !cmdlineopts.readreps_file.empty() ? "--read_repeats"
                              : !cmdlineopts.profile_file.empty() ? "--profile_out" : !o.dump.empty() ? "--dump_jobs" : !o.dist_dump.empty() ? "--dump_dist" : !o.joins_dump.empty() ? "--dump_joins"
                              : o.bootstrap.any() ? "--bootstrap"
                              : o.guidance.any() ? "--guidance"
                              : o.mltree.any() ? "--ml_tree" : nullptr;
        if (refused) { std::cerr << "ERROR:--batch cannot be combined with " << refused << std::endl; return 2; }
    }
    if (cmdlineopts.sequence_file.empty() && o.batch_list.empty()) { usage(); return 1; }
    if (o.bootstrap.any()) {
        // (the cutoff is a number in [0, 1): text that is no number, a NaN and everything outside are refused)
        cutoff_ok = cutoff_ok && o.bootstrap.cutoff >= 0.0 && o.bootstrap.cutoff < 1.0;
        const char *why = !o.bootstrap.given && !o.bootstrap.out_given
                              ? (o.bootstrap.any_taxa() ? "--bootstrap_taxa, --bootstrap_taxa_cutoff and --bootstrap_taxa_edges need --bootstrap and --bootstrap_out"
                                                        : "--bootstrap_tbe and --bootstrap_trees need --bootstrap and --bootstrap_out")
                          : o.bootstrap.given != o.bootstrap.out_given ? "--bootstrap and --bootstrap_out need each other"
                          : (o.bootstrap.n < 1 || o.bootstrap.n > 1000) ? "--bootstrap takes a number of replicates from 1 to 1000"
                          : (o.bootstrap.any_taxa() && o.bootstrap.taxa.empty()) ? "--bootstrap_taxa_cutoff and --bootstrap_taxa_edges need --bootstrap_taxa"
                          : !cutoff_ok ? "--bootstrap_taxa_cutoff takes a number X with 0 <= X < 1"
                          : cmdlineopts.wlsrefine_flag ? "--bootstrap cannot be combined with -W"
                          : cmdlineopts.reroot_flag ? "--bootstrap cannot be combined with -r"
                          : !o.topo_file.empty() ? "--bootstrap cannot be combined with --topology" : nullptr;
        if (why) { std::cerr << "ERROR:" << why << std::endl; return 2; }
    }
    if (o.guidance.any()) {
        const char *why = o.guidance.given != o.guidance.out_given ? "--guidance and --guidance_out need each other"
                          : !o.guidance.given ? "--guidance_residues and --guidance_dump need --guidance"
                          : (o.guidance.n < 1 || o.guidance.n > 1000) ? "--guidance takes a number of replicates from 1 to 1000"
                          : cmdlineopts.onlytree_flag ? "--guidance cannot be combined with -T (there is no alignment to score)"
                          : cmdlineopts.wlsrefine_flag ? "--guidance cannot be combined with -W"
                          : cmdlineopts.reroot_flag ? "--guidance cannot be combined with -r"
                          : !o.topo_file.empty() ? "--guidance cannot be combined with --topology (every replicate would have the same topology)" : nullptr;
        if (why) { std::cerr << "ERROR:" << why << std::endl; return 2; }
    }
    if (o.mltree.any()) {
        // (the rounds are a whole number in 1 .. 10000, the gain a finite number >= 0, the categories a whole number in 2 .. 16, the
        // shape a number in [0.05, 100]: other text, a NaN and everything outside are refused; a default is within its range)
        rounds_ok = rounds_ok && o.mltree.rounds >= 1 && o.mltree.rounds <= 10000;
        eps_ok = eps_ok && o.mltree.eps >= 0.0 && o.mltree.eps < INFINITY;
        gamma_ok = !o.mltree.gamma_given || (gamma_ok && o.mltree.gamma >= 2 && o.mltree.gamma <= PGM_TREELIK_MAXCAT);
        alpha_ok = alpha_ok && o.mltree.alpha >= kMlMinAlpha && o.mltree.alpha <= kMlMaxAlpha;
        search_ok = !o.mltree.search_given || (search_ok && o.mltree.search >= 1 && o.mltree.search <= 1000);
        reps_ok = reps_ok && o.mltree.support_reps >= 1 && o.mltree.support_reps <= 10000;
        nni_opt_ok = !o.mltree.nni_opt_given || (nni_opt_ok && o.mltree.nni_opt >= 1 && o.mltree.nni_opt <= 20);
        spr_ok = !o.mltree.spr_given || (spr_ok && o.mltree.spr >= 1 && o.mltree.spr <= 10);
        samples_ok = !o.mltree.samples_given || (samples_ok && o.mltree.samples >= 1 && o.mltree.samples <= 1000);
        const bool plain = o.mltree.sites_given || o.mltree.rounds_given || o.mltree.eps_given;   // (the flags from before --ml_gamma keep their message)
        const bool rates = o.mltree.gamma_given || o.mltree.alpha_given || o.mltree.rates_given;   // (... and so do those from before --ml_ancestral)
        const char *why = !o.mltree.tree_given ? (plain ? "--ml_sites, --ml_rounds and --ml_epsilon need --ml_tree"
                                                  : rates ? "--ml_gamma, --ml_alpha and --ml_rates need --ml_tree"
                                                  : o.mltree.any_anc() ? "--ml_ancestral needs --ml_tree"
                                                  : o.mltree.any_joint() ? "--ml_ancestral_joint and --ml_ancestral_samples need --ml_tree"
                                                  : o.mltree.nni_opt_given ? "--ml_nni_opt needs --ml_tree"
                                                  : o.mltree.spr_given ? "--ml_spr needs --ml_tree"
                                                  : o.mltree.any_search() ? "--ml_search, --ml_start and --ml_search_log need --ml_tree"
                                                                          : "--ml_support, --ml_support_table, --ml_support_reps and --ml_support_seed need --ml_tree")
                          : (!o.mltree.gamma_given && (o.mltree.alpha_given || o.mltree.rates_given)) ? "--ml_alpha and --ml_rates need --ml_gamma"
                          : (!o.mltree.anc_given && o.mltree.any_anc()) ? "--ml_ancestral_tree and --ml_ancestral_probs need --ml_ancestral"
                          : (!o.mltree.joint_given && o.mltree.joint_sites_given) ? "--ml_ancestral_joint_sites needs --ml_ancestral_joint"
                          : o.mltree.samples_given != o.mltree.samples_out_given ? "--ml_ancestral_samples and --ml_ancestral_samples_out need each other"
                          : (!o.mltree.samples_given && o.mltree.samples_seed_given) ? "--ml_ancestral_samples_seed needs --ml_ancestral_samples"
                          : !samples_ok ? "--ml_ancestral_samples takes a number of samples from 1 to 1000"
                          : !samples_seed_ok ? "--ml_ancestral_samples_seed takes a whole number from 0 to 18446744073709551615"
                          : (!o.mltree.search_given && o.mltree.search_log_given) ? "--ml_search_log needs --ml_search"
                          : (!o.mltree.support_given && o.mltree.any_support()) ? "--ml_support_table, --ml_support_reps and --ml_support_seed need --ml_support"
                          : (o.mltree.nni_opt_given && !o.mltree.search_given && !o.mltree.support_given) ? "--ml_nni_opt needs --ml_search or --ml_support"
                          : !nni_opt_ok ? "--ml_nni_opt takes a number of rounds from 1 to 20"
                          : (o.mltree.spr_given && !o.mltree.search_given) ? "--ml_spr needs --ml_search"
                          : !spr_ok ? "--ml_spr takes a radius from 1 to 10"
                          : !reps_ok ? "--ml_support_reps takes a number of replicates from 1 to 10000"
                          : !search_ok ? "--ml_search takes a number of rounds from 1 to 1000"
                          : !gamma_ok ? "--ml_gamma takes a number of categories from 2 to 16"
                          : !alpha_ok ? "--ml_alpha takes a number X with 0.05 <= X <= 100"
                          : !rounds_ok ? "--ml_rounds takes a number of rounds from 1 to 10000"
                          : !eps_ok ? "--ml_epsilon takes a number X >= 0"
                          : cmdlineopts.wlsrefine_flag ? "--ml_tree cannot be combined with -W"
                          : cmdlineopts.reroot_flag ? "--ml_tree cannot be combined with -r"
                          : !o.topo_file.empty() ? "--ml_tree cannot be combined with --topology" : nullptr;
        if (why) { std::cerr << "ERROR:" << why << std::endl; return 2; }
    }
    if (cmdlineopts.reroot_flag && (cmdlineopts.ancestral_flag || !cmdlineopts.profile_file.empty())) {
        std::cerr << "ERROR:--ancestral_seqs and --profile_out cannot be combined with -r (the root search keeps no ancestral profiles)" << std::endl;
        return 2;
    }
    if (cmdlineopts.dna_flag && (cmdlineopts.codon_flag || !cmdlineopts.cs_file.empty())) {
        std::cerr << "ERROR:--dna cannot be combined with " << (cmdlineopts.codon_flag ? "--codon" : "-c (context-specific profiles are amino-acid profiles)") << std::endl;
        return 2;
    }
    if (cmdlineopts.codon_flag) {  // main.cpp:225-241
        if (!o.indel_set) cmdlineopts.indel_rate /= 2.6;
        if (!o.edgehl_set) cmdlineopts.edge_halflife *= 2.6;
        if (!o.maxdist_set) cmdlineopts.max_dist = 5.0;
        if (!o.cutdist_set) cmdlineopts.cutoff_dist = 5.0;
    }
    // main.cpp:243-246; this build also cannot iterate (see doAlign), so -a/-T runs behave as `-i 0`
    if (!o.iters_set && !cmdlineopts.tree_file.empty()) cmdlineopts.iters = 0;   // do not iterate when a guide tree is provided (main.cpp:243-246)
    return -1;
}

}  // namespace pgm
