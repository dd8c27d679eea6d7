// main.cpp — command-line driver mirroring the reference's main()/doAlign (src/main.cpp:32-483) for
// the flags the hot path's configurations use.  TCLAP is not available, so a minimal parser accepts
// the same spellings.  Built twice: `pgmsa` (HIP backend, the product) and, for tests only,
// `oracle/_build/pgmsa_oracle` (CPU oracle backend).
#include "pgm_host.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <malloc.h>
#include <sstream>
#include <unistd.h>
#include <string>
#include <thread>

using namespace pgm;

static void usage() {
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

// The backend (device contexts: the HIP runtime's start-up takes 80-400 ms) is created on a thread of its own while the
// sequences are read and the models are set up; doAlign waits for it before the clocks of the stages start.
namespace {
struct BackendStartup {
    std::thread thr;
    double seconds = 0;
    std::string err;
    void start() {
        thr = std::thread([this]() {
            const auto t0 = std::chrono::steady_clock::now();
            try { default_backend(); }
            catch (std::exception &e) { err = e.what(); }
            seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        });
    }
    void wait() {
        if (thr.joinable()) thr.join();
        if (!err.empty()) throw pgm_exception(err);
    }
    ~BackendStartup() { if (thr.joinable()) thr.join(); }
} g_startup;
}  // namespace

static std::string value_name(const Alphabet &a, int j) {   // ALPHABET(j).asString()
    static const char *aa = "ACDEFGHIKLMNPQRSTVWY";
    if (a.kind == ALPHA_AA) return std::string(1, aa[j]);
    static const char nt[] = "TCAG";
    if (a.kind == ALPHA_DNA) return std::string(1, nt[j]);   // dna_inv_translation_table
    int k = -1;
    for (int c = 0; c < 64; ++c) {
        const std::string cod = {nt[c >> 4], nt[(c >> 2) & 3], nt[c & 3]};
        if (cod == "TAA" || cod == "TAG" || cod == "TGA") continue;
        if (++k == j) return cod;
    }
    return "?";
}

// What doAlign keeps for one family (main.cpp:332-482): the solo run is this state for one family, `--batch` walks the states of
// a chunk of families through the same stages together.
namespace {
struct Family {
    std::string input, output, tree_file, topo_file;   // (--batch: the fields of the family's line of the list)
    int iters = 0;
    std::vector<std::string> input_order;
    std::map<std::string, std::string> seqs;   // as read
    bool any_start = false, any_end = false;
    std::map<std::string, bool> startStripped, endStripped;
    std::map<std::string, sequence_t> seqs2;   // start / stop stripped
    std::unique_ptr<ModelFactory> model_factory;   // (per family: -F estimates the frequencies from the family's sequences)
    PhyTree *tree = nullptr;
    PhyTree *topo = nullptr;   // --topology: every estimated tree keeps this topology
    ProgressiveAlignmentResult result, old_result;
    bool done = false;   // converged: takes no further part in the iterations
    std::string failure;   // --batch: the message the solo run would have ended with
    double cells = 0;    // --batch: estimated DP cells of one pass
    int worker = 0;
    std::map<std::string, std::string> aligned;
    ~Family() { delete tree; delete topo; }

    // strip start/stop (main.cpp:332-353) and set the models up
    void prepare(const Alphabet &a) {
        for (const auto &kv : seqs) {
            sequence_t seq = sequenceFromString(a, kv.second);
            if (!cmdlineopts.noforcealign_flag) {
                if (!seq.empty() && a.stripsStart(seq[0])) { seq = seq.substr(1); any_start = true; startStripped[kv.first] = true; }
                else startStripped[kv.first] = false;
                if (!seq.empty() && a.stripsEnd(seq[seq.size() - 1])) { seq = seq.substr(0, seq.size() - 1); any_end = true; endStripped[kv.first] = true; }
                else endStripped[kv.first] = false;
            }
            seqs2[kv.first] = seq;
        }
        model_factory.reset(ModelFactory::getDefault(a, seqs2));
    }
    void read_tree() {
        std::ifstream ts(tree_file.c_str());
        if (!ts) error("cannot open tree file %s", tree_file.c_str());
        tree = parse_newick(ts);
    }
    void read_topology() {   // (main.cpp:384-387)
        std::ifstream ts(topo_file.c_str());
        if (!ts) error("cannot open topology file %s", topo_file.c_str());
        topo = parse_newick(ts);
    }
    void drop_ancestral_rows() {
        for (auto it = result.aligned_sequences.begin(); it != result.aligned_sequences.end();)   // ancestral sequences
            if (!it->first.empty() && it->first[0] == '(') it = result.aligned_sequences.erase(it); else ++it;
    }
    // re-insert start/stop (main.cpp:459-482): a row as it is written, one symbol a column (ancestral rows were never stripped)
    sequence_t written_row(const Alphabet &a, const std::string &name, sequence_t aseq) const {
        const auto st = startStripped.find(name), en = endStripped.find(name);
        if (any_start) aseq.insert(aseq.begin(), st != startStripped.end() && st->second ? a.unknown() : a.gap());
        if (any_end) aseq.insert(aseq.end(), en != endStripped.end() && en->second ? a.unknown() : a.gap());
        return aseq;
    }
    void finish_rows(const Alphabet &a, const std::map<std::string, sequence_t> &rows, std::map<std::string, std::string> &out) const {
        for (const auto &kv : rows) {
            const sequence_t aseq = written_row(a, kv.first, kv.second);
            out[kv.first] = seqs.count(kv.first) ? stringFromSequence(a, aseq, seqs.at(kv.first)) : stringFromSequence(a, aseq);   // (ancestral rows have no original)
        }
    }
    void finish(const Alphabet &a) { finish_rows(a, result.aligned_sequences, aligned); }
    void write(std::ostream &out) const {
        if (!cmdlineopts.onlytree_flag) {
            std::vector<std::string> order = input_order;
            if (!cmdlineopts.inputorder_flag) order = get_tree_order(tree);
            write_fasta(aligned, order, out);
        } else {
            out << tree->formatNewick() << std::endl;
        }
    }
};

struct BatchRun { int families = 0, failed = 0, chunks = 0; };

struct BootstrapOpts {   // --bootstrap N --bootstrap_out FILE --bootstrap_seed S
    bool given = false, out_given = false;
    long long n = 0;
    std::string out, tbe, trees;   // --bootstrap_tbe FILE, --bootstrap_trees FILE
    std::string taxa, taxa_edges, cutoff_text;   // --bootstrap_taxa FILE, --bootstrap_taxa_edges FILE, --bootstrap_taxa_cutoff X
    bool cutoff_given = false;
    double cutoff = 0.3;
    uint64_t seed = 1;
    bool any_taxa() const { return !taxa.empty() || !taxa_edges.empty() || cutoff_given; }
    bool any() const { return given || out_given || !tbe.empty() || !trees.empty() || any_taxa(); }
} g_bootstrap;

struct GuidanceOpts {   // --guidance N --guidance_out FILE --guidance_seed S --guidance_residues FILE --guidance_dump PREFIX
    bool given = false, out_given = false;
    long long n = 0;
    std::string out, residues, dump;
    uint64_t seed = 1;
    double cells = 2e9;   // --batch_cells: estimated DP cells of one group of replicates
} g_guidance;

struct MlTreeOpts {   // --ml_tree FILE --ml_sites FILE --ml_rounds N --ml_epsilon X --ml_gamma K --ml_alpha X --ml_rates FILE
    std::string tree, sites, rounds_text, eps_text, gamma_text, alpha_text, rates;
    bool tree_given = false, sites_given = false, rounds_given = false, eps_given = false, gamma_given = false, alpha_given = false, rates_given = false;
    long rounds = 100, gamma = 0;
    double eps = 1e-4, alpha = 1.0;
    bool any() const { return tree_given || sites_given || rounds_given || eps_given || gamma_given || alpha_given || rates_given; }
} g_mltree;
}  // namespace

static void doGuidance(const Alphabet &a, const Family &fam, const CSProfile *csprofile, const std::map<std::string, std::vector<repeat_t>> &reps);

// --bootstrap: the tree TreeNJ estimates from the final alignment without its ancestral rows (the re-estimation step of the
// iterations: main.cpp:404-430, DistanceFactoryPrealigned.h:34-90, TreeNJ.h:27-59), the support of its internal edges among the
// trees of N column resamplings, and the file: formatNewick()'s text with the counts as node labels.  --bootstrap_tbe: the same
// text with the transfer bootstrap expectation of every labelled node (transfer_support; the device from kTransferDeviceMin taxa
// or with PGM_DEVICE_TRANSFER, the host loop with PGM_HOST_TRANSFER); --bootstrap_trees: formatNewick() of every replicate's tree;
// --bootstrap_taxa / --bootstrap_taxa_edges: taxa_support by the same route, taxa_text and taxa_edges_text
static void doBootstrap(const Alphabet &a, const Family &fam, const std::map<std::string, sequence_t> &alignment) {
    const auto t0 = std::chrono::steady_clock::now();
    std::map<std::string, sequence_t> rows;
    for (const auto &kv : alignment)
        if (kv.first.empty() || kv.first[0] != '(') rows.insert(kv);   // (ancestral sequences dropped)
    std::unique_ptr<PhyTree> tree(TreeNJ(a, rows, fam.model_factory.get(), true));
    std::vector<PhyTree *> reps = bootstrap_trees(a, rows, fam.model_factory.get(), (uint32_t)g_bootstrap.n, g_bootstrap.seed);
    std::string text, tbe_text, trees_text, taxa_file_text, taxa_edges_file_text;
    try {
        const std::vector<const PhyTree *> replicates(reps.begin(), reps.end());
        text = tree->formatNewick(bipartition_support(*tree, replicates));
        const HostSwitches &sw = host_switches();
        const bool device = !sw.host_transfer && (sw.device_transfer || rows.size() >= kTransferDeviceMin);
        if (!g_bootstrap.tbe.empty())
            tbe_text = tree->formatNewick(transfer_labels(transfer_support(*tree, replicates, device ? &default_backend() : nullptr), (uint32_t)replicates.size()));
        if (!g_bootstrap.taxa.empty()) {
            const TaxaSupport taxa = taxa_support(*tree, replicates, g_bootstrap.cutoff, device ? &default_backend() : nullptr);
            taxa_file_text = taxa_text(taxa, g_bootstrap.cutoff);
            if (!g_bootstrap.taxa_edges.empty()) taxa_edges_file_text = taxa_edges_text(taxa);
        }
        if (!g_bootstrap.trees.empty())
            for (const PhyTree *t : replicates) trees_text += t->formatNewick() + "\n";
    } catch (...) {
        for (PhyTree *t : reps) delete t;
        throw;
    }
    for (PhyTree *t : reps) delete t;
    std::ofstream out(g_bootstrap.out.c_str());
    if (!out) error("error opening the bootstrap output file %s", g_bootstrap.out.c_str());
    out << text << std::endl;
    if (!g_bootstrap.tbe.empty()) {
        std::ofstream tbe(g_bootstrap.tbe.c_str());
        if (!tbe) error("error opening the bootstrap output file %s", g_bootstrap.tbe.c_str());
        tbe << tbe_text << std::endl;
    }
    if (!g_bootstrap.trees.empty()) {
        std::ofstream trees(g_bootstrap.trees.c_str());
        if (!trees) error("error opening the bootstrap output file %s", g_bootstrap.trees.c_str());
        trees << trees_text << std::flush;
    }
    if (!g_bootstrap.taxa.empty()) {
        std::ofstream taxa(g_bootstrap.taxa.c_str());
        if (!taxa) error("error opening the bootstrap output file %s", g_bootstrap.taxa.c_str());
        taxa << taxa_file_text << std::flush;
    }
    if (!g_bootstrap.taxa_edges.empty()) {
        std::ofstream edges(g_bootstrap.taxa_edges.c_str());
        if (!edges) error("error opening the bootstrap output file %s", g_bootstrap.taxa_edges.c_str());
        edges << taxa_edges_file_text << std::flush;
    }
    bootstrap_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// --ml_tree: the tree of --bootstrap (TreeNJ on the final alignment without its ancestral rows, midpoint rooted) with the branch
// lengths that maximise the likelihood of the alignment as it is written (start / stop columns re-inserted, every residue the
// character of the input: Family::finish_rows), and --ml_sites: the log-likelihood of every column (ml_branch_lengths, DESIGN.md
// 3.17; the device from kTreelikDeviceMin taxa or with PGM_DEVICE_TREELIK, the host loop with PGM_HOST_TREELIK).  With --ml_gamma the
// likelihood is the mixture over the rate categories of the discrete gamma (the same route), and --ml_rates: the
// shape, the categories' rates, and per column the posterior mean rate and the category of the largest posterior
static void doMlTree(const Alphabet &a, const Family &fam, const std::map<std::string, sequence_t> &alignment) {
    std::map<std::string, sequence_t> rows;
    for (const auto &kv : alignment)
        if (kv.first.empty() || kv.first[0] != '(') rows.insert(kv);   // (ancestral sequences dropped)
    std::unique_ptr<PhyTree> tree(TreeNJ(a, rows, fam.model_factory.get(), true));
    std::vector<std::vector<int8_t>> values;   // the rows in sorted-name order: the leaves' order
    for (const auto &kv : rows) {
        const sequence_t written = fam.written_row(a, kv.first, kv.second), orig = sequenceFromString(a, fam.seqs.at(kv.first));
        std::vector<int8_t> v(written.size());
        size_t j = 0;
        for (size_t k = 0; k < written.size(); ++k) {
            if (a.isGap(written[k])) { v[k] = -1; continue; }
            const int x = j < orig.size() ? a.value(orig[j]) : -1;
            ++j;
            v[k] = (int8_t)(x >= 0 && x < a.DIM ? x : -2);
        }
        values.push_back(std::move(v));
    }
    const HostSwitches &sw = host_switches();
    const bool device = !sw.host_treelik && (sw.device_treelik || rows.size() >= kTreelikDeviceMin);
    MlGamma gamma;
    if (g_mltree.gamma_given) { gamma.ncat = (uint32_t)g_mltree.gamma; gamma.estimate = !g_mltree.alpha_given; gamma.alpha = g_mltree.alpha; }
    const MlTreeResult res = ml_branch_lengths(a, values, *fam.model_factory, *tree, (uint32_t)g_mltree.rounds, g_mltree.eps, device ? &default_backend() : nullptr, gamma);
    std::unique_ptr<PhyTree> ml(ml_tree_with_lengths(ml_tree_topology(*tree), res.lengths));
    std::ofstream out(g_mltree.tree.c_str());
    if (!out) error("error opening the ml tree output file %s", g_mltree.tree.c_str());
    out << ml->formatNewick() << std::endl;
    if (g_mltree.sites_given) {
        std::ofstream sites(g_mltree.sites.c_str());
        if (!sites) error("error opening the ml tree output file %s", g_mltree.sites.c_str());
        char buf[64];
        snprintf(buf, sizeof buf, "lnL %.17g\n", res.lnl);
        sites << buf;
        for (size_t c = 0; c < res.site_lnl.size(); ++c) {
            snprintf(buf, sizeof buf, "%zu\t%.17g\n", c + 1, res.site_lnl[c]);
            sites << buf;
        }
    }
    if (g_mltree.rates_given) {
        std::ofstream rates(g_mltree.rates.c_str());
        if (!rates) error("error opening the ml tree output file %s", g_mltree.rates.c_str());
        char buf[96];
        snprintf(buf, sizeof buf, "alpha\t%.17g\n", res.alpha);
        rates << buf;
        const size_t ncat = res.rates.size(), ncols = res.site_lnl.size();
        for (size_t k = 0; k < ncat; ++k) {
            snprintf(buf, sizeof buf, "rate\t%zu\t%.17g\n", k + 1, res.rates[k]);
            rates << buf;
        }
        for (size_t c = 0; c < ncols; ++c) {   // the posterior mean rate, categories ascending; the first category of the largest posterior
            double mean = 0.0;
            size_t top = 0;
            for (size_t k = 0; k < ncat; ++k) {
                mean = mean + res.post[k * ncols + c] * res.rates[k];
                if (res.post[k * ncols + c] > res.post[top * ncols + c]) top = k;
            }
            snprintf(buf, sizeof buf, "%zu\t%.17g\t%zu\n", c + 1, mean, top + 1);
            rates << buf;
        }
    }
}

static void print_stats(double t_init, double t_tree, double t_prog, const BatchRun *batch) {
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
    if (g_bootstrap.given)   // (keys of --bootstrap only)
        fprintf(stderr, ", \"bootstrap_replicates\": %d, \"bootstrap_s\": %.6f, \"bootstrap_counts_calls\": %llu", bootstrap_stats.replicates, bootstrap_stats.seconds,
                (unsigned long long)bootstrap_stats.counts_calls);
    if (!g_bootstrap.tbe.empty())   // (keys of --bootstrap_tbe only)
        fprintf(stderr, ", \"bootstrap_tbe_s\": %.6f, \"bootstrap_transfer_calls\": %llu, \"bootstrap_transfer_kernel_ms\": %.3f", transfer_stats.seconds,
                (unsigned long long)transfer_stats.calls, transfer_stats.kernel_ms);
    if (!g_bootstrap.taxa.empty())   // (keys of --bootstrap_taxa only)
        fprintf(stderr, ", \"bootstrap_taxa_s\": %.6f, \"bootstrap_taxa_calls\": %llu, \"bootstrap_taxa_kernel_ms\": %.3f", taxa_stats.seconds,
                (unsigned long long)taxa_stats.calls, taxa_stats.kernel_ms);
    if (g_guidance.given)   // (keys of --guidance only)
        fprintf(stderr, ", \"guidance_replicates\": %d, \"guidance_s\": %.6f, \"guidance_align_s\": %.6f, \"guidance_agreement_s\": %.6f, "
                        "\"guidance_passes\": %llu, \"guidance_agreement_calls\": %llu",
                guidance_stats.replicates, guidance_stats.seconds, guidance_stats.align_s, guidance_stats.agreement_s, (unsigned long long)guidance_stats.passes,
                (unsigned long long)guidance_stats.agreement_calls);
    if (g_mltree.tree_given)   // (keys of --ml_tree only)
        fprintf(stderr, ", \"ml_tree_s\": %.6f, \"ml_rounds\": %llu, \"ml_evaluations\": %llu, \"ml_lnl_start\": %.17g, \"ml_lnl\": %.17g, \"ml_kernel_ms\": %.3f",
                ml_tree_stats.seconds, (unsigned long long)ml_tree_stats.rounds, (unsigned long long)ml_tree_stats.evaluations, ml_tree_stats.lnl_start, ml_tree_stats.lnl,
                ml_tree_stats.kernel_ms);
    if (g_mltree.gamma_given)   // (keys of --ml_gamma only)
        fprintf(stderr, ", \"ml_categories\": %u, \"ml_alpha\": %.17g", ml_tree_stats.categories, ml_tree_stats.alpha);
    if (batch)   // (keys of --batch only)
        fprintf(stderr, ", \"batch_families\": %d, \"batch_failed\": %d, \"batch_chunks\": %d, \"batch_passes\": %llu, \"batch_levels\": %llu, "
                        "\"batch_align_calls\": %llu, \"batch_dist_calls\": %llu",
                batch->families, batch->failed, batch->chunks, (unsigned long long)batch_stats.passes, (unsigned long long)batch_stats.levels,
                (unsigned long long)be.calls_align.load(), (unsigned long long)be.calls_dist.load());
    fprintf(stderr, "}\n");
}

// the device contexts (HIP runtime start-up, code object load) exist before the clocks of the stages start; init_s is the
// time their creation took (it ran beside the set-up), init_wait_s what of it was left to wait for here
static double wait_for_backend(const CSProfile *csprofile) {
    auto t0 = std::chrono::steady_clock::now();
    g_startup.wait();
    default_backend();
    double t_preload = 0;
    if (csprofile) {   // the profile library goes to the devices with the rest of the start-up (counted in init_s)
        const auto tp = std::chrono::steady_clock::now();
        default_backend().csprofile_preload(*csprofile);
        t_preload = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
    }
    const double t_init = (g_startup.seconds > 0 ? g_startup.seconds : std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()) + t_preload;
    if (host_switches().profile)
        fprintf(stderr, "backend start-up %.1f ms, of which %.1f ms waited for after the set-up\n", t_init * 1e3,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return t_init;
}

static int doAlign(const Alphabet &a, Family &fam, bool stats) {
    fam.prepare(a);
    std::unique_ptr<CSProfile> csprofile;
    if (!cmdlineopts.cs_file.empty()) csprofile.reset(new CSProfile(cmdlineopts.cs_file));
    const double t_init = wait_for_backend(csprofile.get());
    std::map<std::string, std::vector<repeat_t>> reps;   // main.cpp:367-370 (detection by T-REKS itself is not built here: --read_repeats only)
    if (!cmdlineopts.readreps_file.empty()) reps = read_repeats(a, cmdlineopts.readreps_file, fam.seqs2);
    auto t0 = std::chrono::steady_clock::now();
    if (!fam.topo_file.empty()) fam.read_topology();
    if (!fam.tree_file.empty()) fam.read_tree();
    else fam.tree = TreeNJ(a, fam.seqs2, fam.model_factory.get(), false, fam.topo);
    double t_tree = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ProgressiveAlignmentResult &result = fam.result;
    t0 = std::chrono::steady_clock::now();
    // further rounds of alignment followed by estimation of an improved tree from the induced pairwise distances
    // (main.cpp:404-430; the default is two such rounds when no tree is given)
    for (int i = 0; i < fam.iters; ++i) {
        result = progressive_alignment(a, fam.seqs2, *fam.tree, csprofile.get(), *fam.model_factory, &reps);
        fam.drop_ancestral_rows();
        if (i > 0 && result.aligned_sequences == fam.old_result.aligned_sequences) break;   // converged
        delete fam.tree;
        fam.tree = nullptr;
        const auto tt0 = std::chrono::steady_clock::now();
        fam.tree = TreeNJ(a, result.aligned_sequences, fam.model_factory.get(), true, fam.topo);
        if (host_switches().profile) fprintf(stderr, "guide tree from the alignment: %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tt0).count());
        fam.old_result = result;
    }
    // the final alignment (main.cpp:433-440): with -r the guide tree rerooted on the branch of the lowest gap parsimony
    if (!cmdlineopts.onlytree_flag)
        result = cmdlineopts.reroot_flag ? progressive_alignment_find_root(a, fam.seqs2, *fam.tree, *fam.model_factory, &reps)
                                         : progressive_alignment(a, fam.seqs2, *fam.tree, csprofile.get(), *fam.model_factory, &reps);
    if (host_switches().profile) fprintf(stderr, "[%.1f ms] back in main\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    double t_prog = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (g_bootstrap.given) {   // (with -T the final alignment is computed for it alone: what is printed stays the tree)
        if (cmdlineopts.onlytree_flag) doBootstrap(a, fam, progressive_alignment(a, fam.seqs2, *fam.tree, csprofile.get(), *fam.model_factory, &reps).aligned_sequences);
        else doBootstrap(a, fam, result.aligned_sequences);
    }
    if (g_mltree.tree_given) {   // (with -T the final alignment is computed for it alone, as for --bootstrap)
        if (cmdlineopts.onlytree_flag) doMlTree(a, fam, progressive_alignment(a, fam.seqs2, *fam.tree, csprofile.get(), *fam.model_factory, &reps).aligned_sequences);
        else doMlTree(a, fam, result.aligned_sequences);
    }
    if (g_guidance.given) doGuidance(a, fam, csprofile.get(), reps);

    fam.finish(a);
    if (cmdlineopts.repeats_flag) {
        if (cmdlineopts.readreps_file.empty()) error("-R: tandem-repeat detection (T-REKS, a Java program) is not built here; supply the repeats with --read_repeats");
        std::cerr << "TR indels: " << result.n_tr_indels << std::endl;   // main.cpp:447-449
    }
    if (!cmdlineopts.profile_file.empty()) {   // write_profile (profile.h:12-31; main.cpp:451-456): default stream formatting, 6 significant digits
        std::ofstream pf(cmdlineopts.profile_file.c_str());
        for (const auto &kv : result.profiles) {
            pf << '>' << kv.first << std::endl;
            for (int j = 0; j < a.DIM; ++j) {
                pf << value_name(a, j);
                for (index_t k = 0; k < kv.second.cols; ++k) pf << '\t' << kv.second.data[(size_t)j + (size_t)a.DIM * k];
                pf << std::endl;
            }
        }
    }
    if (stats) print_stats(t_init, t_tree, t_prog, nullptr);
    return 0;
}

// ---- --batch ----------------------------------------------------------------------------------------------------------
// Estimated DP cells of one pass over a family: the sum over the internal nodes of its tree of (residues below the left child) x
// (residues below the right child) — an over-estimate that needs no alignment —, (N - 1) x (mean length)^2 before a tree exists.
static double subtree_cells(const PhyTree &t, const std::map<std::string, sequence_t> &seqs, double &cells) {
    if (t.isLeaf()) { auto it = seqs.find(t.getName()); return it == seqs.end() ? 0.0 : (double)it->second.size(); }
    std::vector<double> below;
    double sum = 0;
    for (index_t c = 0; c < t.n_children(); ++c) { below.push_back(subtree_cells(t[(int)c], seqs, cells)); sum += below.back(); }
    if (below.size() == 2) cells += below[0] * below[1];
    return sum;
}
static double estimate_cells(const Family &fam) {
    double cells = 0;
    if (fam.tree) { subtree_cells(*fam.tree, fam.seqs2, cells); return cells; }
    if (fam.seqs2.empty()) return 0;
    double total = 0;
    for (const auto &kv : fam.seqs2) total += (double)kv.second.size();
    const double mean = total / (double)fam.seqs2.size();
    return ((double)fam.seqs2.size() - 1.0) * mean * mean;
}

// One forest pass over the families of `act`; a family the pass refuses gets its message and leaves the run.
static void forest_pass(const Alphabet &a, const std::vector<Family *> &act, const CSProfile *csprofile) {
    std::vector<ForestFamily> ff(act.size());
    for (size_t k = 0; k < act.size(); ++k) {
        ff[k].sequences = &act[k]->seqs2; ff[k].tree = act[k]->tree; ff[k].model_factory = act[k]->model_factory.get();
        ff[k].result = &act[k]->result; ff[k].worker = act[k]->worker;
    }
    progressive_alignment_forest(a, ff, csprofile);
    for (size_t k = 0; k < act.size(); ++k) if (!ff[k].error.empty()) act[k]->failure = ff[k].error;
}
static void trees_for(const Alphabet &a, const std::vector<Family *> &act, bool prealigned) {
    std::vector<TreeJob> jobs(act.size());
    for (size_t k = 0; k < act.size(); ++k) {
        jobs[k].seqs = prealigned ? &act[k]->result.aligned_sequences : &act[k]->seqs2;
        jobs[k].model_factory = act[k]->model_factory.get();
        jobs[k].topo = act[k]->topo;
    }
    TreeNJ_multi(a, jobs, prealigned);
    for (size_t k = 0; k < act.size(); ++k) {
        if (!jobs[k].error.empty()) act[k]->failure = jobs[k].error;
        else act[k]->tree = jobs[k].tree;
    }
}
static std::vector<Family *> alive(const std::vector<Family *> &v) {
    std::vector<Family *> out;
    for (Family *f : v) if (f->failure.empty()) out.push_back(f);
    return out;
}

// --guidance (Penn et al. 2010, GUIDANCE: the guide tree as the source of alignment uncertainty): the final alignment's columns are
// resampled N times as --bootstrap resamples them, every replicate's BioNJ tree, midpoint rooted and written with exact branch
// lengths, is read back as `-t` reads a tree and used as the guide tree of a realignment of the family's sequences (forest passes
// over groups of replicates within --batch_cells), and Backend::msa_agreement counts per group how often the residue pairs of the
// alignment as written (start / stop columns re-inserted, ancestral rows left out) share a column in the replicates' alignments.
static void doGuidance(const Alphabet &a, const Family &fam, const CSProfile *csprofile, const std::map<std::string, std::vector<repeat_t>> &reps) {
    typedef std::chrono::steady_clock clk;
    const auto t0 = clk::now();
    Backend &be = default_backend();
    const uint32_t N = (uint32_t)g_guidance.n;
    std::map<std::string, sequence_t> rows;
    for (const auto &kv : fam.result.aligned_sequences)
        if (kv.first.empty() || kv.first[0] != '(') rows.insert(kv);   // (ancestral sequences dropped)
    if (rows.size() < 4) error("--guidance needs at least 4 sequences");
    std::vector<std::string> names;
    std::vector<sequence_t> base;
    for (const auto &kv : rows) { names.push_back(kv.first); base.push_back(fam.written_row(a, kv.first, kv.second)); }
    const size_t n = names.size(), L = base[0].size();
    if (L == 0 || L > 0x7fffffffull) error("guidance: an alignment of %zu columns", L);

    // the replicates' guide trees
    std::vector<std::unique_ptr<PhyTree>> trees(N);
    {
        const BootstrapStats kept = bootstrap_stats;   // (the keys of --bootstrap count its own replicates only)
        std::vector<PhyTree *> unrooted = bootstrap_trees(a, rows, fam.model_factory.get(), N, g_guidance.seed);
        bootstrap_stats = kept;
        for (uint32_t r = 0; r < N; ++r) trees[r].reset(unrooted[r]);
        for (uint32_t r = 0; r < N; ++r) {
            trees[r].reset(midpointRoot(trees[r].release()));
            const std::string text = format_newick_exact(*trees[r]);
            if (!g_guidance.dump.empty()) {
                const std::string path = g_guidance.dump + "." + std::to_string(r) + ".nwk";
                std::ofstream out(path.c_str());
                if (!out) error("error opening the guidance dump file %s", path.c_str());
                out << text << std::endl;
            }
            std::istringstream in(text);
            trees[r].reset(parse_newick(in));   // (as -t reads it: every branch support 1)
        }
    }
    // groups of replicates in order while the estimated cells of a pass stay within the bound; a larger replicate alone
    std::vector<double> cells(N, 0.0);
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    {
        double sum = 0;
        for (uint32_t r = 0; r < N; ++r) {
            subtree_cells(*trees[r], fam.seqs2, cells[r]);
            if (groups.empty() || sum + cells[r] > g_guidance.cells) { groups.emplace_back(r, r); sum = 0; }
            ++groups.back().second;
            sum += cells[r];
        }
    }
    GuidanceCounts G;
    G.nrows = (uint32_t)n; G.ncols = (uint32_t)L; G.nrep = N;
    G.res_hits.assign(n * L, 0); G.pair_hits.assign(n * n, 0);
    const uint32_t per_call = guidance_call_replicates(G.nrows, G.ncols);
    std::vector<int32_t> where;
    std::vector<uint32_t> res32(n * L), pair32(n * n);
    for (const auto &grp : groups) {
        const uint32_t g = grp.second - grp.first;
        const auto ta = clk::now();
        std::vector<ProgressiveAlignmentResult> res(g);
        {
            std::vector<ForestFamily> ff(g);
            std::vector<uint64_t> cost(g);
            for (uint32_t k = 0; k < g; ++k) {
                ff[k].sequences = &fam.seqs2; ff[k].tree = trees[grp.first + k].get(); ff[k].model_factory = fam.model_factory.get();
                ff[k].repeats = &reps; ff[k].result = &res[k];
                cost[k] = (uint64_t)cells[grp.first + k] + 1u;
            }
            const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, be.workers());   // (as run_chunk deals families)
            for (size_t w = 0; w < shards.size(); ++w) for (uint32_t k : shards[w]) ff[k].worker = (int)w;
            progressive_alignment_forest(a, ff, csprofile);
            ++guidance_stats.passes;
            for (uint32_t k = 0; k < g; ++k) if (!ff[k].error.empty()) throw pgm_exception(ff[k].error);
        }
        guidance_stats.align_s += std::chrono::duration<double>(clk::now() - ta).count();
        std::vector<std::vector<sequence_t>> written(g);
        parallel_for(g, [&](size_t k) {
            for (const std::string &name : names) {
                const auto it = res[k].aligned_sequences.find(name);
                if (it == res[k].aligned_sequences.end()) error("guidance: a replicate alignment without sequence %s", name.c_str());
                written[k].push_back(fam.written_row(a, name, it->second));
            }
            if (!g_guidance.dump.empty()) {   // the replicate's alignment as `-t <its tree>` writes it
                const uint32_t r = grp.first + (uint32_t)k;
                std::map<std::string, std::string> aligned;
                fam.finish_rows(a, res[k].aligned_sequences, aligned);
                const std::string path = g_guidance.dump + "." + std::to_string(r) + ".fa";
                std::ofstream out(path.c_str());
                if (!out) error("error opening the guidance dump file %s", path.c_str());
                write_fasta(aligned, cmdlineopts.inputorder_flag ? fam.input_order : get_tree_order(trees[r].get()), out);
            }
            res[k] = ProgressiveAlignmentResult();
        });
        for (uint32_t k0 = 0; k0 < g; k0 += per_call) {
            const uint32_t m = std::min(per_call, g - k0);
            where.resize((size_t)m * n * L);
            parallel_for(m, [&](size_t k) { guidance_where(a, base, written[k0 + k], where.data() + k * n * L); });
            const auto tg = clk::now();
            be.msa_agreement(G.nrows, G.ncols, m, where.data(), res32.data(), pair32.data());
            guidance_stats.agreement_s += std::chrono::duration<double>(clk::now() - tg).count();
            ++guidance_stats.agreement_calls;
            for (size_t k = 0; k < res32.size(); ++k) G.res_hits[k] += res32[k];
            for (size_t k = 0; k < pair32.size(); ++k) G.pair_hits[k] += pair32[k];
        }
    }
    std::vector<int32_t> where0(n * L);   // (the gaps of the base alignment)
    for (size_t i = 0; i < n; ++i)
        for (size_t c = 0; c < L; ++c) where0[i * L + c] = a.isGap(base[i][c]) ? -1 : 0;
    std::ofstream out(g_guidance.out.c_str());
    if (!out) error("error opening the guidance output file %s", g_guidance.out.c_str());
    std::ofstream rout;
    if (!g_guidance.residues.empty()) {
        rout.open(g_guidance.residues.c_str());
        if (!rout) error("error opening the guidance residue file %s", g_guidance.residues.c_str());
    }
    guidance_write(G, names, where0.data(), g_guidance.seed, out, g_guidance.residues.empty() ? nullptr : &rout);
    guidance_stats.replicates += (int)N;
    guidance_stats.seconds += std::chrono::duration<double>(clk::now() - t0).count();
}

// The families of a chunk through the stages of doAlign in lock-step: every device stage once for all of them.
static void run_chunk(const Alphabet &a, const std::vector<Family *> &chunk, const CSProfile *csprofile) {
    {   // the families dealt to the device contexts, longest first (a family never spans contexts)
        std::vector<uint64_t> cost(chunk.size());
        for (size_t k = 0; k < chunk.size(); ++k) cost[k] = (uint64_t)chunk[k]->cells + 1u;
        const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, default_backend().workers());
        for (size_t w = 0; w < shards.size(); ++w) for (uint32_t k : shards[w]) chunk[k]->worker = (int)w;
    }
    // 1. initial trees
    std::vector<Family *> need;
    for (Family *f : chunk) if (!f->tree) need.push_back(f);
    if (!need.empty()) trees_for(a, need, false);
    // 2. rounds of alignment followed by a tree from the alignment (main.cpp:404-430), per family as far as its own loop goes
    int max_iters = 0;
    for (Family *f : chunk) max_iters = std::max(max_iters, f->iters);
    for (int i = 0; i < max_iters; ++i) {
        std::vector<Family *> act;
        for (Family *f : chunk) if (f->failure.empty() && !f->done && i < f->iters) act.push_back(f);
        if (act.empty()) break;
        forest_pass(a, act, csprofile);
        act = alive(act);
        std::vector<Family *> go_on;
        for (Family *f : act) {
            f->drop_ancestral_rows();
            if (i > 0 && f->result.aligned_sequences == f->old_result.aligned_sequences) { f->done = true; continue; }   // converged
            delete f->tree;
            f->tree = nullptr;
            go_on.push_back(f);
        }
        if (!go_on.empty()) trees_for(a, go_on, true);
        for (Family *f : alive(go_on)) f->old_result = f->result;
    }
    // 3. the final alignment
    if (!cmdlineopts.onlytree_flag) forest_pass(a, alive(chunk), csprofile);
}

static int doBatch(const Alphabet &a, const std::string &list_file, bool iters_set, double batch_cells, bool stats) {
    std::vector<std::unique_ptr<Family>> fams;
    {
        std::ifstream in(list_file.c_str());
        if (!in) error("cannot open the list of families %s", list_file.c_str());
        std::string line;
        for (int lineno = 1; std::getline(in, line); ++lineno) {
            if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
            if (line.empty() || line[0] == '#') continue;
            std::vector<std::string> field(1);
            for (char c : line) { if (c == '\t') field.emplace_back(); else field.back() += c; }
            bool blank = true;
            for (char c : line) blank = blank && (c == '\t' || c == ' ');
            if (blank) continue;
            if (field.size() < 2 || field.size() > 4 || field[0].empty() || field[1].empty())
                error("--batch: line %d of %s: expected input<TAB>output[<TAB>tree[<TAB>topology]], found %zu field(s)", lineno, list_file.c_str(), field.size());
            std::unique_ptr<Family> f(new Family);
            f->input = field[0]; f->output = field[1];
            if (field.size() >= 3) f->tree_file = field[2];
            if (field.size() == 4) f->topo_file = field[3];
            f->iters = (!iters_set && !f->tree_file.empty()) ? 0 : cmdlineopts.iters;   // no iterations with a guide tree (main.cpp:243-246)
            fams.push_back(std::move(f));
        }
    }
    BatchRun run;
    run.families = (int)fams.size();
    g_startup.start();
    parallel_for(64, [](size_t) {});   // (the driver's host threads start while the device runtime does)
    std::unique_ptr<CSProfile> csprofile;
    if (!cmdlineopts.cs_file.empty()) csprofile.reset(new CSProfile(cmdlineopts.cs_file));
    parallel_for(fams.size(), [&](size_t k) {
        Family &f = *fams[k];
        try {
            f.seqs = read_fasta(f.input, f.input_order);
            f.prepare(a);
            if (!f.tree_file.empty()) f.read_tree();
            if (!f.topo_file.empty()) f.read_topology();
            f.cells = estimate_cells(f);
        } catch (std::exception &e) { f.failure = e.what(); }
    });
    const double t_init = wait_for_backend(csprofile.get());
    const auto t0 = std::chrono::steady_clock::now();
    auto report = [&](Family &f) {
        std::cerr << "family " << f.input << ": ERROR:" << f.failure << std::endl;
        ++run.failed;
    };
    // chunks: families in list order while the estimated cells of a pass stay within the bound; a larger family alone
    std::vector<std::vector<Family *>> chunks;
    {
        double cells = 0;
        for (auto &f : fams) {
            if (!f->failure.empty()) continue;
            if (chunks.empty() || (!chunks.back().empty() && cells + f->cells > batch_cells)) { chunks.emplace_back(); cells = 0; }
            chunks.back().push_back(f.get());
            cells += f->cells;
        }
    }
    run.chunks = (int)chunks.size();
    for (auto &f : fams) if (!f->failure.empty()) report(*f);
    for (const std::vector<Family *> &chunk : chunks) {
        try { run_chunk(a, chunk, csprofile.get()); }
        catch (std::exception &e) { for (Family *f : chunk) if (f->failure.empty()) f->failure = e.what(); }   // (a stage all its families share)
        const std::vector<Family *> ok = alive(chunk);
        parallel_for(ok.size(), [&](size_t k) {
            Family &f = *ok[k];
            try {
                f.finish(a);
                std::ofstream out(f.output.c_str());
                if (!out) error("error opening output file");
                f.write(out);
            } catch (std::exception &e) { f.failure = e.what(); }
        });
        for (Family *f : chunk) {
            if (!f->failure.empty()) report(*f);
            f->seqs.clear(); f->seqs2.clear(); f->aligned.clear();
            f->result = ProgressiveAlignmentResult(); f->old_result = ProgressiveAlignmentResult();
            delete f->tree; f->tree = nullptr;
            delete f->topo; f->topo = nullptr;
            f->model_factory.reset();
        }
    }
    const double t_prog = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) print_stats(t_init, 0.0, t_prog, &run);
    return run.failed ? 2 : 0;
}

int main(int argc, char **argv) {
    const auto t_main = std::chrono::steady_clock::now();
    // The graphs of a level are hundreds of vectors of 0.1-1 MB built and dropped by the host threads: with glibc's defaults
    // each is an mmap / munmap of its own (page faults on every reuse, the address-space lock shared by all threads), and
    // the heap is trimmed back to the system whenever its top is freed.  Keep them in the heaps instead.
    if (!getenv("PGM_MALLOC_DEFAULTS")) {
        mallopt(M_MMAP_THRESHOLD, 1 << 30);
        mallopt(M_TRIM_THRESHOLD, 0x7fffffff);
        mallopt(M_TOP_PAD, 64 << 20);
    }
    try {
        bool iters_set = false, stats = false, indel_set = false, edgehl_set = false, maxdist_set = false, cutdist_set = false;
        std::string dump, dist_dump, joins_dump, batch_list, topo_file;
        double batch_cells = 2e9;
        for (int i = 1; i < argc; ++i) {
            std::string s = argv[i];
            auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); exit(1); } return argv[++i]; };
            if (s == "-f" || s == "--fasta") cmdlineopts.fasta_flag = true;
            else if (s == "-t" || s == "--tree") cmdlineopts.tree_file = val();
            else if (s == "--topology") topo_file = val();
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
            else if (s == "-i" || s == "--iterations") { cmdlineopts.iters = atoi(val().c_str()); iters_set = true; }
            else if (s == "-g" || s == "--indel_rate") { cmdlineopts.indel_rate = atof(val().c_str()); indel_set = true; }
            else if (s == "-e" || s == "--gap_ext") cmdlineopts.gapext_prob = atof(val().c_str());
            else if (s == "-E" || s == "--end_indel_prob") cmdlineopts.end_indel_prob = atof(val().c_str());
            else if (s == "-s" || s == "--altsplice_prob") cmdlineopts.altsplice_prob = atof(val().c_str());
            else if (s == "-l" || s == "--edge_halflife") { cmdlineopts.edge_halflife = atof(val().c_str()); edgehl_set = true; }
            else if (s == "-x" || s == "--cutoff_dist") { cmdlineopts.cutoff_dist = atof(val().c_str()); cutdist_set = true; }
            else if (s == "-d" || s == "--min_dist") cmdlineopts.min_dist = atof(val().c_str());
            else if (s == "-D" || s == "--max_dist") { cmdlineopts.max_dist = atof(val().c_str()); maxdist_set = true; }
            else if (s == "-p" || s == "--min_pdist") cmdlineopts.min_pdist = atof(val().c_str());
            else if (s == "-P" || s == "--max_pdist") cmdlineopts.max_pdist = atof(val().c_str());
            else if (s == "--ancestral_seqs") cmdlineopts.ancestral_flag = true;
            else if (s == "--early_refinement") cmdlineopts.earlyref_flag = true;
            else if (s == "--profile_out") cmdlineopts.profile_file = val();
            else if (s == "--read_repeats") cmdlineopts.readreps_file = val();
            else if (s == "-R" || s == "--repeats") cmdlineopts.repeats_flag = true;
            else if (s == "--dump_jobs") dump = val();
            else if (s == "--dump_dist") dist_dump = val();
            else if (s == "--dump_joins") joins_dump = val();
            else if (s == "--stats") stats = true;
            else if (s == "--batch") batch_list = val();
            else if (s == "--batch_cells") batch_cells = atof(val().c_str());
            else if (s == "--bootstrap") { g_bootstrap.given = true; g_bootstrap.n = atoll(val().c_str()); }
            else if (s == "--bootstrap_out") { g_bootstrap.out_given = true; g_bootstrap.out = val(); }
            else if (s == "--bootstrap_seed") g_bootstrap.seed = strtoull(val().c_str(), nullptr, 10);
            else if (s == "--bootstrap_tbe") g_bootstrap.tbe = val();
            else if (s == "--bootstrap_trees") g_bootstrap.trees = val();
            else if (s == "--bootstrap_taxa") g_bootstrap.taxa = val();
            else if (s == "--bootstrap_taxa_edges") g_bootstrap.taxa_edges = val();
            else if (s == "--bootstrap_taxa_cutoff") { g_bootstrap.cutoff_given = true; g_bootstrap.cutoff_text = val(); g_bootstrap.cutoff = atof(g_bootstrap.cutoff_text.c_str()); }
            else if (s == "--guidance") { g_guidance.given = true; g_guidance.n = atoll(val().c_str()); }
            else if (s == "--guidance_out") { g_guidance.out_given = true; g_guidance.out = val(); }
            else if (s == "--guidance_seed") g_guidance.seed = strtoull(val().c_str(), nullptr, 10);
            else if (s == "--guidance_residues") g_guidance.residues = val();
            else if (s == "--guidance_dump") g_guidance.dump = val();
            else if (s == "--ml_tree") { g_mltree.tree_given = true; g_mltree.tree = val(); }
            else if (s == "--ml_sites") { g_mltree.sites_given = true; g_mltree.sites = val(); }
            else if (s == "--ml_rounds") { g_mltree.rounds_given = true; g_mltree.rounds_text = val(); }
            else if (s == "--ml_epsilon") { g_mltree.eps_given = true; g_mltree.eps_text = val(); }
            else if (s == "--ml_gamma") { g_mltree.gamma_given = true; g_mltree.gamma_text = val(); }
            else if (s == "--ml_alpha") { g_mltree.alpha_given = true; g_mltree.alpha_text = val(); }
            else if (s == "--ml_rates") { g_mltree.rates_given = true; g_mltree.rates = val(); }
            else if (s == "--reroot") ++cmdlineopts.reroot_flag;
            else if (s == "--wls_refine") ++cmdlineopts.wlsrefine_flag;
            else if (s.size() >= 2 && s[0] == '-' && s.find_first_not_of('W', 1) == std::string::npos) cmdlineopts.wlsrefine_flag += (int)s.size() - 1;   // -W, -WW
            else if (s.size() >= 2 && s[0] == '-' && s.find_first_not_of('r', 1) == std::string::npos) cmdlineopts.reroot_flag += (int)s.size() - 1;   // -r, -rr (TCLAP's MultiSwitchArg)
            else if (s == "-h" || s == "--help") { usage(); return 0; }
            else if (!s.empty() && s[0] == '-') { std::cerr << "Command line error: unknown flag " << s << std::endl; return 1; }
            else cmdlineopts.sequence_file = s;
        }
        if (!batch_list.empty()) {   // what belongs to one family or is a search loop of its own is refused
            const char *refused = !cmdlineopts.sequence_file.empty() ? "a positional sequence file (the families come from the list)"
                                  : !cmdlineopts.output_file.empty() ? "-o (every line of the list names its output)"
                                  : !cmdlineopts.tree_file.empty() ? "-t (a guide tree is the third field of a family's line)"
                                  : !topo_file.empty() ? "--topology (a topology is the fourth field of a family's line)"
                                  : cmdlineopts.reroot_flag ? "-r" : cmdlineopts.wlsrefine_flag ? "-W"
                                  : cmdlineopts.repeats_flag ? "-R" : !cmdlineopts.readreps_file.empty() ? "--read_repeats"
                                  : !cmdlineopts.profile_file.empty() ? "--profile_out" : !dump.empty() ? "--dump_jobs" : !dist_dump.empty() ? "--dump_dist" : !joins_dump.empty() ? "--dump_joins"
                                  : g_bootstrap.any() ? "--bootstrap"
                                  : (g_guidance.given || g_guidance.out_given || !g_guidance.residues.empty() || !g_guidance.dump.empty()) ? "--guidance"
                                  : g_mltree.any() ? "--ml_tree" : nullptr;
            if (refused) { std::cerr << "ERROR:--batch cannot be combined with " << refused << std::endl; return 2; }
        }
        if (cmdlineopts.sequence_file.empty() && batch_list.empty()) { usage(); return 1; }
        if (g_bootstrap.any()) {
            // (the cutoff is a number in [0, 1): text that is no number, a NaN and everything outside are refused)
            char *cutoff_end = nullptr;
            if (g_bootstrap.cutoff_given) (void)strtod(g_bootstrap.cutoff_text.c_str(), &cutoff_end);
            const bool cutoff_ok = !g_bootstrap.cutoff_given || (!g_bootstrap.cutoff_text.empty() && *cutoff_end == '\0' && g_bootstrap.cutoff >= 0.0 && g_bootstrap.cutoff < 1.0);
            const char *why = !g_bootstrap.given && !g_bootstrap.out_given
                                  ? (g_bootstrap.any_taxa() ? "--bootstrap_taxa, --bootstrap_taxa_cutoff and --bootstrap_taxa_edges need --bootstrap and --bootstrap_out"
                                                            : "--bootstrap_tbe and --bootstrap_trees need --bootstrap and --bootstrap_out")
                              : g_bootstrap.given != g_bootstrap.out_given ? "--bootstrap and --bootstrap_out need each other"
                              : (g_bootstrap.n < 1 || g_bootstrap.n > 1000) ? "--bootstrap takes a number of replicates from 1 to 1000"
                              : (g_bootstrap.any_taxa() && g_bootstrap.taxa.empty()) ? "--bootstrap_taxa_cutoff and --bootstrap_taxa_edges need --bootstrap_taxa"
                              : !cutoff_ok ? "--bootstrap_taxa_cutoff takes a number X with 0 <= X < 1"
                              : cmdlineopts.wlsrefine_flag ? "--bootstrap cannot be combined with -W"
                              : cmdlineopts.reroot_flag ? "--bootstrap cannot be combined with -r"
                              : !topo_file.empty() ? "--bootstrap cannot be combined with --topology" : nullptr;
            if (why) { std::cerr << "ERROR:" << why << std::endl; return 2; }
        }
        if (g_guidance.given || g_guidance.out_given || !g_guidance.residues.empty() || !g_guidance.dump.empty()) {
            const char *why = g_guidance.given != g_guidance.out_given ? "--guidance and --guidance_out need each other"
                              : !g_guidance.given ? "--guidance_residues and --guidance_dump need --guidance"
                              : (g_guidance.n < 1 || g_guidance.n > 1000) ? "--guidance takes a number of replicates from 1 to 1000"
                              : cmdlineopts.onlytree_flag ? "--guidance cannot be combined with -T (there is no alignment to score)"
                              : cmdlineopts.wlsrefine_flag ? "--guidance cannot be combined with -W"
                              : cmdlineopts.reroot_flag ? "--guidance cannot be combined with -r"
                              : !topo_file.empty() ? "--guidance cannot be combined with --topology (every replicate would have the same topology)" : nullptr;
            if (why) { std::cerr << "ERROR:" << why << std::endl; return 2; }
            g_guidance.cells = batch_cells;
        }
        if (g_mltree.any()) {
            // (the rounds are a whole number in 1 .. 10000, the gain a finite number >= 0: other text, a NaN and everything outside are refused)
            char *end = nullptr;
            bool rounds_ok = true, eps_ok = true, gamma_ok = true, alpha_ok = true;
            if (g_mltree.rounds_given) {
                g_mltree.rounds = strtol(g_mltree.rounds_text.c_str(), &end, 10);
                rounds_ok = !g_mltree.rounds_text.empty() && *end == '\0' && g_mltree.rounds >= 1 && g_mltree.rounds <= 10000;
            }
            if (g_mltree.eps_given) {
                g_mltree.eps = strtod(g_mltree.eps_text.c_str(), &end);
                eps_ok = !g_mltree.eps_text.empty() && *end == '\0' && g_mltree.eps >= 0.0 && g_mltree.eps < INFINITY;
            }
            if (g_mltree.gamma_given) {   // (the categories are a whole number in 2 .. 16, the shape a number in [0.05, 100])
                g_mltree.gamma = strtol(g_mltree.gamma_text.c_str(), &end, 10);
                gamma_ok = !g_mltree.gamma_text.empty() && *end == '\0' && g_mltree.gamma >= 2 && g_mltree.gamma <= PGM_TREELIK_MAXCAT;
            }
            if (g_mltree.alpha_given) {
                g_mltree.alpha = strtod(g_mltree.alpha_text.c_str(), &end);
                alpha_ok = !g_mltree.alpha_text.empty() && *end == '\0' && g_mltree.alpha >= kMlMinAlpha && g_mltree.alpha <= kMlMaxAlpha;
            }
            const bool plain = g_mltree.sites_given || g_mltree.rounds_given || g_mltree.eps_given;   // (the flags from before --ml_gamma keep their message)
            const char *why = !g_mltree.tree_given ? (plain ? "--ml_sites, --ml_rounds and --ml_epsilon need --ml_tree" : "--ml_gamma, --ml_alpha and --ml_rates need --ml_tree")
                              : (!g_mltree.gamma_given && (g_mltree.alpha_given || g_mltree.rates_given)) ? "--ml_alpha and --ml_rates need --ml_gamma"
                              : !gamma_ok ? "--ml_gamma takes a number of categories from 2 to 16"
                              : !alpha_ok ? "--ml_alpha takes a number X with 0.05 <= X <= 100"
                              : !rounds_ok ? "--ml_rounds takes a number of rounds from 1 to 10000"
                              : !eps_ok ? "--ml_epsilon takes a number X >= 0"
                              : cmdlineopts.wlsrefine_flag ? "--ml_tree cannot be combined with -W"
                              : cmdlineopts.reroot_flag ? "--ml_tree cannot be combined with -r"
                              : !topo_file.empty() ? "--ml_tree cannot be combined with --topology" : nullptr;
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
            if (!indel_set) cmdlineopts.indel_rate /= 2.6;
            if (!edgehl_set) cmdlineopts.edge_halflife *= 2.6;
            if (!maxdist_set) cmdlineopts.max_dist = 5.0;
            if (!cutdist_set) cmdlineopts.cutoff_dist = 5.0;
        }
        // main.cpp:243-246; this build also cannot iterate (see doAlign), so -a/-T runs behave as `-i 0`
        if (!iters_set && !cmdlineopts.tree_file.empty()) cmdlineopts.iters = 0;   // do not iterate when a guide tree is provided (main.cpp:243-246)
        if (!dump.empty()) set_job_dump(dump);
        if (!dist_dump.empty()) set_dist_dump(dist_dump);
        if (!joins_dump.empty()) set_joins_dump(joins_dump);
        if (!batch_list.empty()) {
            Alphabet a(cmdlineopts.codon_flag ? ALPHA_CODON : cmdlineopts.dna_flag ? ALPHA_DNA : ALPHA_AA);
            if (!cmdlineopts.fasta_flag && !cmdlineopts.onlytree_flag) std::cerr << "note: Stockholm output is not built here; writing FASTA" << std::endl;
            const int rc = doBatch(a, batch_list, iters_set, batch_cells, stats);
            if (!getenv("PGM_FULL_EXIT") && std::string(default_backend().name()) == "hip") {   // (as below: the outputs are complete)
                std::cout.flush(); std::cerr.flush(); fflush(nullptr);
                _exit(rc);
            }
            return rc;
        }

        g_startup.start();
        parallel_for(64, [](size_t) {});   // (the driver's host threads start while the device runtime does)
        Family fam;
        fam.input = cmdlineopts.sequence_file; fam.tree_file = cmdlineopts.tree_file; fam.topo_file = topo_file; fam.iters = cmdlineopts.iters;
        fam.seqs = read_fasta(cmdlineopts.sequence_file, fam.input_order);
        if (g_bootstrap.given && fam.seqs.size() < 4) error("--bootstrap needs at least 4 sequences");
        if (g_guidance.given && fam.seqs.size() < 4) error("--guidance needs at least 4 sequences");
        if (g_mltree.tree_given && fam.seqs.size() < 3) error("--ml_tree needs at least 3 sequences");
        std::ofstream custom_out;
        std::ostream *out = &std::cout;
        if (!cmdlineopts.output_file.empty()) {
            custom_out.open(cmdlineopts.output_file.c_str());
            if (!custom_out) error("error opening output file");
            out = &custom_out;
        }
        Alphabet a(cmdlineopts.codon_flag ? ALPHA_CODON : cmdlineopts.dna_flag ? ALPHA_DNA : ALPHA_AA);
        doAlign(a, fam, stats);
        if (!cmdlineopts.onlytree_flag && !cmdlineopts.fasta_flag) std::cerr << "note: Stockholm output is not built here; writing FASTA" << std::endl;
        fam.write(*out);
        if (host_switches().profile)
            fprintf(stderr, "main: output written %.1f ms after its start\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_main).count());
        // The output is complete.  Releasing the contexts' gigabytes of device memory and pinned blocks and shutting the HIP runtime
        // down in an orderly way takes 30-70 ms that the kernel driver spends anyway when the process is gone: leave directly
        // (PGM_FULL_EXIT=1 for runs under a profiler or a sanitizer, whose reports are written by exit handlers).
        if (!getenv("PGM_FULL_EXIT") && std::string(default_backend().name()) == "hip") {
            custom_out.close();
            std::cout.flush(); std::cerr.flush(); fflush(nullptr);
            _exit(0);
        }
    } catch (std::exception &e) {
        std::cerr << "ERROR:" << e.what() << std::endl;
        return 2;
    }
    return 0;
}
