// driver_analyses.cpp — what the solo run computes from its final alignment besides writing it: --bootstrap, --ml_tree, --guidance.
#include "driver.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <set>
#include <sstream>

namespace pgm {

// the alignment's rows without the ancestral sequences
static std::map<std::string, sequence_t> sequence_rows(const std::map<std::string, sequence_t> &alignment) {
    std::map<std::string, sequence_t> rows;
    for (const auto &kv : alignment)
        if (kv.first.empty() || kv.first[0] != '(') rows.insert(kv);
    return rows;
}
// `what`: "bootstrap output", "ml tree output", "guidance output", "guidance residue", "guidance dump"
static std::ofstream open_output(const std::string &path, const char *what) {
    std::ofstream out(path.c_str());
    if (!out) error("error opening the %s file %s", what, path.c_str());
    return out;
}

// --bootstrap: the tree TreeNJ estimates from the final alignment without its ancestral rows (the re-estimation step of the
// iterations: main.cpp:404-430, DistanceFactoryPrealigned.h:34-90, TreeNJ.h:27-59), the support of its internal edges among the
// trees of N column resamplings, and the file: formatNewick()'s text with the counts as node labels.  --bootstrap_tbe: the same
// text with the transfer bootstrap expectation of every labelled node (transfer_support; the device from kTransferDeviceMin taxa
// or with PGM_DEVICE_TRANSFER, the host loop with PGM_HOST_TRANSFER); --bootstrap_trees: formatNewick() of every replicate's tree;
// --bootstrap_taxa / --bootstrap_taxa_edges: taxa_support by the same route, taxa_text and taxa_edges_text
void doBootstrap(const Alphabet &a, const DriverOptions &o, const Family &fam, const std::map<std::string, sequence_t> &alignment) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::map<std::string, sequence_t> rows = sequence_rows(alignment);
    std::unique_ptr<PhyTree> tree(TreeNJ(a, rows, fam.model_factory.get(), true));
    const BootstrapOpts &bo = o.bootstrap;
    std::vector<PhyTree *> reps = bootstrap_trees(a, rows, fam.model_factory.get(), (uint32_t)bo.n, bo.seed);
    std::string text, tbe_text, trees_text, taxa_file_text, taxa_edges_file_text;
    try {
        const std::vector<const PhyTree *> replicates(reps.begin(), reps.end());
        text = tree->formatNewick(bipartition_support(*tree, replicates));
        const HostSwitches &sw = host_switches();
        Backend *device = !sw.host_transfer && (sw.device_transfer || rows.size() >= kTransferDeviceMin) ? &default_backend() : nullptr;
        if (!bo.tbe.empty())
            tbe_text = tree->formatNewick(transfer_labels(transfer_support(*tree, replicates, device), (uint32_t)replicates.size()));
        if (!bo.taxa.empty()) {
            const TaxaSupport taxa = taxa_support(*tree, replicates, bo.cutoff, device);
            taxa_file_text = taxa_text(taxa, bo.cutoff);
            if (!bo.taxa_edges.empty()) taxa_edges_file_text = taxa_edges_text(taxa);
        }
        if (!bo.trees.empty())
            for (const PhyTree *t : replicates) trees_text += t->formatNewick() + "\n";
    } catch (...) {
        for (PhyTree *t : reps) delete t;
        throw;
    }
    for (PhyTree *t : reps) delete t;
    open_output(bo.out, "bootstrap output") << text << std::endl;
    if (!bo.tbe.empty()) open_output(bo.tbe, "bootstrap output") << tbe_text << std::endl;
    if (!bo.trees.empty()) open_output(bo.trees, "bootstrap output") << trees_text << std::flush;
    if (!bo.taxa.empty()) open_output(bo.taxa, "bootstrap output") << taxa_file_text << std::flush;
    if (!bo.taxa_edges.empty()) open_output(bo.taxa_edges, "bootstrap output") << taxa_edges_file_text << std::flush;
    bootstrap_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// --ml_tree: the tree of --bootstrap (TreeNJ on the final alignment without its ancestral rows, midpoint rooted) with the branch
// lengths that maximise the likelihood of the alignment as it is written (start / stop columns re-inserted, every residue the
// character of the input: Family::finish_rows), and --ml_sites: the log-likelihood of every column (ml_branch_lengths, DESIGN.md
// 3.17; the device from kTreelikDeviceMin taxa or with PGM_DEVICE_TREELIK, the host loop with PGM_HOST_TREELIK).  With --ml_gamma the
// likelihood is the mixture over the rate categories of the discrete gamma (the same route), and --ml_rates: the
// shape, the categories' rates, and per column the posterior mean rate and the category of the largest posterior.
// --ml_ancestral: one Backend::tree_ancestral call at the estimated lengths (and rates) by the same route, and the
// FASTA of the inner nodes' most probable states; --ml_ancestral_tree: the tree with the nodes' names; --ml_ancestral_probs: a line
// per node and column; --ml_ancestral_joint and --ml_ancestral_samples: the jointly most probable states and draws
// from the posterior, by the same route.  --ml_search N: up to N rounds of nearest-neighbour interchanges from the start tree, every
// candidate of a round scored by one Backend::tree_nni call (the same route); --ml_start FILE: a newick in place of the BioNJ tree;
// --ml_search_log FILE: a line per round; --ml_nni_opt N: the candidates of the search and of --ml_support each at a
// central length of their own, N Newton rounds by Backend::tree_nni_edge calls (the same route); --ml_spr R: where the
// interchanges of a round apply no move, every pruning and regrafting within R edges scored by Backend::tree_spr calls (the same
// route), and a ninth column, nni or spr, in every line of the log
// the names of the inner nodes of a numbered tree, N1 .. in node order; a leaf that has one of them is an error()
static std::vector<std::string> ml_ancestral_names(const MlTreeTopology &topo, const char *flag = "--ml_ancestral") {
    std::vector<std::string> node_name(topo.nnodes - topo.nleaves);
    for (size_t k = 0; k < node_name.size(); ++k) node_name[k] = "N" + std::to_string(k + 1);
    const std::set<std::string> taken(node_name.begin(), node_name.end());
    for (const std::string &leaf : topo.names)
        if (taken.count(leaf)) error("%s: the sequence name %s is the name of an inner node", flag, leaf.c_str());
    return node_name;
}
// What the files of the inner nodes' states share (--ml_ancestral, --ml_ancestral_joint, --ml_ancestral_samples): the numbered tree,
// the rows, the categories' weights and matrices at the estimated lengths (and rates), and the text of a state under the gap rule.
struct MlNodeStates {
    MlTreeTopology topo;
    uint32_t dim, nleaves, nnodes, ninner, ncols, ncat;
    std::vector<std::string> node_name;
    std::vector<int8_t> flat;
    std::vector<double> w, P;
    const double *pi;
    std::vector<uint8_t> present;      // tree_ancestral_presence
    std::vector<std::string> symbol;   // the character(s) of a state: the alphabet's own symbol (the first letter that has the value; a codon's three)
    std::string gap;
    MlNodeStates(const Alphabet &a, const Family &fam, const PhyTree &ml, const std::vector<std::vector<int8_t>> &values, const MlTreeResult &res, const char *flag)
        : topo(ml_tree_topology(ml)), dim((uint32_t)a.DIM), nleaves(topo.nleaves), nnodes(topo.nnodes), ninner(nnodes - nleaves), ncols((uint32_t)values[0].size()),
          ncat(res.rates.empty() ? 1u : (uint32_t)res.rates.size()), node_name(ml_ancestral_names(topo, flag)), flat((size_t)nleaves * ncols),
          w(ncat, res.rates.empty() ? 1.0 : 1.0 / (double)ncat), pi(fam.model_factory->freqs().data()), present((size_t)ninner * ncols, 0), symbol(dim),
          gap(a.rawChars() ? a.asString(a.gap()) : "---") {
        for (uint32_t r = 0; r < nleaves; ++r) std::copy(values[r].begin(), values[r].end(), flat.begin() + (size_t)r * ncols);
        tree_ancestral_presence(nleaves, nnodes, topo.parent.data(), ncols, flat.data(), present.data());
        for (uint32_t x = 0; x < dim; ++x) {
            if (!a.rawChars()) { symbol[x] = a.asString((int8_t)x); continue; }
            for (char ch = 'A'; ch <= 'Z' && symbol[x].empty(); ++ch)
                if (a.value((int8_t)ch) == (int)x) symbol[x] = std::string(1, ch);
        }
    }
    // the categories' rates at the estimated shape and equal weights, or one category of weight 1.0 and the plain matrices
    void matrices(const Family &fam, const MlTreeResult &res) {
        if (res.rates.empty()) treelik_matrices(*fam.model_factory, res.lengths, false, P);
        else treelik_matrices(*fam.model_factory, res.lengths, false, res.rates, P);
    }
    const std::string &text_of(int8_t x, bool held) const { return held && x >= 0 ? symbol[(size_t)x] : gap; }
    bool held(uint32_t k, uint32_t s) const { return present[(size_t)k * ncols + s] != 0; }
};
static void write_ml_ancestral(const Alphabet &a, const MlTreeOpts &mo, const Family &fam, const PhyTree &ml, const std::vector<std::vector<int8_t>> &values,
                               const MlTreeResult &res, Backend *be) {
    MlNodeStates n(a, fam, ml, values, res, "--ml_ancestral");
    const uint32_t ninner = n.ninner, ncols = n.ncols;
    const auto t0 = std::chrono::steady_clock::now();   // (ml_ancestral_s: the matrices and the call)
    n.matrices(fam, res);
    std::vector<double> site_l(ncols), post((size_t)n.ncat * ncols), prob((size_t)ninner * ncols);
    std::vector<int32_t> site_k(ncols);
    std::vector<int8_t> state((size_t)ninner * ncols);
    if (be) be->tree_ancestral(n.dim, n.nleaves, n.nnodes, n.topo.parent.data(), ncols, n.flat.data(), n.pi, n.ncat, n.w.data(), n.P.data(), site_l.data(), site_k.data(),
                               post.data(), state.data(), prob.data(), nullptr);
    else tree_ancestral_host(n.dim, n.nleaves, n.nnodes, n.topo.parent.data(), ncols, n.flat.data(), n.pi, n.ncat, n.w.data(), n.P.data(), site_l.data(), site_k.data(),
                             post.data(), state.data(), prob.data(), nullptr);
    ml_tree_stats.ancestral_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::map<std::string, std::string> records;
    for (uint32_t k = 0; k < ninner; ++k) {
        std::string &seq = records[n.node_name[k]];
        for (uint32_t s = 0; s < ncols; ++s) seq += n.text_of(state[(size_t)k * ncols + s], n.held(k, s));
    }
    std::ofstream out = open_output(mo.anc, "ml ancestral output");
    write_fasta(records, n.node_name, out);
    if (mo.anc_tree_given) {
        std::map<const PhyTree *, std::string> labels;
        for (uint32_t k = 0; k < ninner; ++k) labels[n.topo.node[n.nleaves + k]] = n.node_name[k];
        open_output(mo.anc_tree, "ml ancestral output") << ml.formatNewick(labels) << std::endl;
    }
    if (mo.anc_probs_given) {
        std::ofstream probs = open_output(mo.anc_probs, "ml ancestral output");
        char buf[64];
        for (uint32_t k = 0; k < ninner; ++k)
            for (uint32_t s = 0; s < ncols; ++s) {
                snprintf(buf, sizeof buf, "\t%u\t%s\t%.17g\t%d\n", s + 1, n.text_of(state[(size_t)k * ncols + s], true).c_str(), prob[(size_t)k * ncols + s], n.held(k, s) ? 1 : 0);
                probs << n.node_name[k] << buf;
            }
    }
}

// --ml_ancestral_joint: one Backend::tree_ancestral_joint call by the same route, the FASTA of the inner nodes' jointly
// most probable states under the gap rule of --ml_ancestral, and --ml_ancestral_joint_sites: `lnJ <sum>`, then per column
// column<TAB>category (from 1)<TAB>log(joint_l) - 256 ln 2 joint_k
static void write_ml_joint(const Alphabet &a, const MlTreeOpts &mo, const Family &fam, const PhyTree &ml, const std::vector<std::vector<int8_t>> &values,
                           const MlTreeResult &res, Backend *be) {
    MlNodeStates n(a, fam, ml, values, res, "--ml_ancestral_joint");
    const uint32_t ninner = n.ninner, ncols = n.ncols;
    const auto t0 = std::chrono::steady_clock::now();   // (ml_ancestral_joint_s: the matrices and the call)
    n.matrices(fam, res);
    std::vector<double> site_l(ncols), post((size_t)n.ncat * ncols), joint_l(ncols);
    std::vector<int32_t> site_k(ncols), joint_k(ncols);
    std::vector<uint8_t> cat(ncols);
    std::vector<int8_t> state((size_t)ninner * ncols);
    if (be) be->tree_ancestral_joint(n.dim, n.nleaves, n.nnodes, n.topo.parent.data(), ncols, n.flat.data(), n.pi, n.ncat, n.w.data(), n.P.data(), site_l.data(), site_k.data(),
                                     post.data(), cat.data(), state.data(), joint_l.data(), joint_k.data());
    else tree_ancestral_joint_host(n.dim, n.nleaves, n.nnodes, n.topo.parent.data(), ncols, n.flat.data(), n.pi, n.ncat, n.w.data(), n.P.data(), site_l.data(), site_k.data(),
                                   post.data(), cat.data(), state.data(), joint_l.data(), joint_k.data());
    ml_tree_stats.ancestral_joint_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::map<std::string, std::string> records;
    for (uint32_t k = 0; k < ninner; ++k) {
        std::string &seq = records[n.node_name[k]];
        for (uint32_t s = 0; s < ncols; ++s) seq += n.text_of(state[(size_t)k * ncols + s], n.held(k, s));
    }
    std::ofstream out = open_output(mo.joint, "ml ancestral output");
    write_fasta(records, n.node_name, out);
    if (mo.joint_sites_given) {
        std::vector<double> site_lnj(ncols);
        const double lnj = treelik_lnl(ncols, joint_l.data(), joint_k.data(), site_lnj.data());
        std::ofstream sites = open_output(mo.joint_sites, "ml ancestral output");
        char buf[96];
        snprintf(buf, sizeof buf, "lnJ %.17g\n", lnj);
        sites << buf;
        for (uint32_t s = 0; s < ncols; ++s) {
            snprintf(buf, sizeof buf, "%u\t%u\t%.17g\n", s + 1, (unsigned)cat[s] + 1, site_lnj[s]);
            sites << buf;
        }
    }
}

// --ml_ancestral_samples N: N draws of every inner node's states from their joint posterior by
// Backend::tree_ancestral_sample calls (the same route), the samples cut into calls whose states stay within kSampleStateBytes; the
// records N<k>/<sample> of --ml_ancestral_samples_out, samples ascending and the nodes of a sample in node order, under the same gap rule
static void write_ml_samples(const Alphabet &a, const MlTreeOpts &mo, const Family &fam, const PhyTree &ml, const std::vector<std::vector<int8_t>> &values,
                             const MlTreeResult &res, Backend *be) {
    MlNodeStates n(a, fam, ml, values, res, "--ml_ancestral_samples");
    const uint32_t ninner = n.ninner, ncols = n.ncols, total = (uint32_t)mo.samples;
    const auto t0 = std::chrono::steady_clock::now();   // (ml_ancestral_samples_s: the matrices, the calls and the records)
    n.matrices(fam, res);
    const uint32_t per_call = (uint32_t)std::min<size_t>(total, std::max<size_t>(1, kSampleStateBytes / ((size_t)ninner * ncols)));
    std::vector<double> site_l(ncols), post((size_t)n.ncat * ncols);
    std::vector<int32_t> site_k(ncols);
    std::vector<uint8_t> cat((size_t)ncols * per_call);
    std::vector<int8_t> state((size_t)ninner * ncols * per_call);
    std::ofstream out = open_output(mo.samples_out, "ml ancestral output");
    std::string text;
    for (uint32_t first = 0; first < total; first += per_call) {
        const uint32_t m = std::min(per_call, total - first);
        if (be) be->tree_ancestral_sample(n.dim, n.nleaves, n.nnodes, n.topo.parent.data(), ncols, n.flat.data(), n.pi, n.ncat, n.w.data(), n.P.data(), m, first, mo.samples_seed,
                                          site_l.data(), site_k.data(), post.data(), cat.data(), state.data());
        else tree_ancestral_sample_host(n.dim, n.nleaves, n.nnodes, n.topo.parent.data(), ncols, n.flat.data(), n.pi, n.ncat, n.w.data(), n.P.data(), m, first, mo.samples_seed,
                                        site_l.data(), site_k.data(), post.data(), cat.data(), state.data());
        for (uint32_t j = 0; j < m; ++j) {
            text.clear();
            for (uint32_t k = 0; k < ninner; ++k) {
                text += ">" + n.node_name[k] + "/" + std::to_string(first + j + 1) + "\n";
                for (uint32_t s = 0; s < ncols; ++s) text += n.text_of(state[((size_t)k * ncols + s) * m + j], n.held(k, s));
                text += "\n";
            }
            out << text;
        }
    }
    out << std::flush;
    ml_tree_stats.ancestral_samples_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// --ml_support: ml_branch_support on the tree the run ends with, at the estimated lengths (and rates), by the same
// route; the tree with %.6f of sh_hits / N as the label of every supported node, and --ml_support_table: a line per supported node
static void write_ml_support(const Alphabet &a, const MlTreeOpts &mo, const Family &fam, const PhyTree &ml, const std::vector<std::vector<int8_t>> &values,
                             const MlTreeResult &res, Backend *be) {
    const MlTreeTopology topo = ml_tree_topology(ml);
    const uint32_t dim = (uint32_t)a.DIM, nleaves = topo.nleaves, nnodes = topo.nnodes, ncols = (uint32_t)values[0].size(), nrep = (uint32_t)mo.support_reps;
    std::vector<int8_t> flat((size_t)nleaves * ncols);
    for (uint32_t r = 0; r < nleaves; ++r) std::copy(values[r].begin(), values[r].end(), flat.begin() + (size_t)r * ncols);
    const uint32_t ncat = res.rates.empty() ? 1u : (uint32_t)res.rates.size();
    const std::vector<double> w(ncat, res.rates.empty() ? 1.0 : 1.0 / (double)ncat);
    std::vector<double> P;
    if (res.rates.empty()) treelik_matrices(*fam.model_factory, res.lengths, false, P);
    else treelik_matrices(*fam.model_factory, res.lengths, false, res.rates, P);
    const std::vector<uint32_t> cols = bootstrap_columns(nrep, ncols, mo.support_seed);
    MlSupportOpt opt;   // --ml_nni_opt: every neighbour at a central length of its own
    opt.rounds = mo.nni_opt_given ? (uint32_t)mo.nni_opt : 0u; opt.mf = fam.model_factory.get(); opt.rates = &res.rates; opt.lengths = &res.lengths;
    const std::vector<MlSupportNode> nodes = ml_branch_support(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), fam.model_factory->freqs().data(), ncat, w.data(),
                                                               P.data(), nrep, cols.data(), be, kSupportBytes, &opt);
    std::map<const PhyTree *, std::string> labels;
    char buf[160];
    for (const MlSupportNode &s : nodes) {
        snprintf(buf, sizeof buf, "%.6f", (double)s.sh_hits / (double)nrep);
        labels[topo.node[s.node]] = buf;
    }
    open_output(mo.support, "ml support output") << ml.formatNewick(labels) << std::endl;
    if (mo.support_table_given) {
        std::ofstream table = open_output(mo.support_table, "ml support output");
        snprintf(buf, sizeof buf, "replicates\t%u\nseed\t%llu\n", nrep, (unsigned long long)mo.support_seed);
        table << buf;
        for (const MlSupportNode &s : nodes) {
            snprintf(buf, sizeof buf, "N%u\t%u\t%.17g\t%u\t%u\n", s.node - nleaves + 1, s.candidates, s.alrt, s.sh_hits, s.rell_hits);
            table << buf;
        }
    }
}

void doMlTree(const Alphabet &a, const DriverOptions &o, const Family &fam, const std::map<std::string, sequence_t> &alignment) {
    const std::map<std::string, sequence_t> rows = sequence_rows(alignment);
    const MlTreeOpts &mo = o.mltree;
    // the start tree: the BioNJ tree of the alignment, or --ml_start's (its lengths go through the optimiser's clamp)
    std::unique_ptr<PhyTree> tree(mo.start_tree ? mo.start_tree->copy() : TreeNJ(a, rows, fam.model_factory.get(), true));
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
    if (mo.gamma_given) { gamma.ncat = (uint32_t)mo.gamma; gamma.estimate = !mo.alpha_given; gamma.alpha = mo.alpha; }
    Backend *be = device ? &default_backend() : nullptr;
    // (a leaf with the name of an inner node is refused before the optimiser runs and before any file is written)
    auto check_node_names = [&]() {
        if (mo.anc_given) (void)ml_ancestral_names(ml_tree_topology(*tree));
        if (mo.joint_given) (void)ml_ancestral_names(ml_tree_topology(*tree), "--ml_ancestral_joint");
        if (mo.samples_given) (void)ml_ancestral_names(ml_tree_topology(*tree), "--ml_ancestral_samples");
    };
    check_node_names();
    MlTreeResult res;
    if (mo.search_given) {   // --ml_search: every file below describes the searched tree
        MlSprHook spr;
        spr.radius = (uint32_t)mo.spr; spr.scan = ml_spr_scan; spr.apply = ml_spr_apply;
        MlSearchResult found = ml_topology_search(a, values, *fam.model_factory, *tree, (uint32_t)mo.search, (uint32_t)mo.rounds, mo.eps, be, gamma,
                                                  mo.nni_opt_given ? (uint32_t)mo.nni_opt : 0u, mo.spr_given ? &spr : nullptr);
        tree = std::move(found.tree);
        res = std::move(found.res);
        check_node_names();
        if (mo.search_log_given) {
            std::ofstream log = open_output(mo.search_log, "ml search output");
            char buf[256];
            for (const MlSearchRound &r : found.log) {
                snprintf(buf, sizeof buf, "%u\t%u\t%u\t%u\t%.17g\t%.17g\t%.17g\t%.17g%s\n", r.round, r.candidates, r.positive, r.applied, r.best_gain, r.lnl_before,
                         r.lnl_applied, r.lnl_after, !mo.spr_given ? "" : r.spr ? "\tspr" : "\tnni");
                log << buf;
            }
        }
    } else res = ml_branch_lengths(a, values, *fam.model_factory, *tree, (uint32_t)mo.rounds, mo.eps, be, gamma);
    std::unique_ptr<PhyTree> ml(ml_tree_with_lengths(ml_tree_topology(*tree), res.lengths));
    open_output(mo.tree, "ml tree output") << ml->formatNewick() << std::endl;
    if (mo.sites_given) {
        std::ofstream sites = open_output(mo.sites, "ml tree output");
        char buf[64];
        snprintf(buf, sizeof buf, "lnL %.17g\n", res.lnl);
        sites << buf;
        for (size_t c = 0; c < res.site_lnl.size(); ++c) {
            snprintf(buf, sizeof buf, "%zu\t%.17g\n", c + 1, res.site_lnl[c]);
            sites << buf;
        }
    }
    if (mo.rates_given) {
        std::ofstream rates = open_output(mo.rates, "ml tree output");
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
    if (mo.anc_given) write_ml_ancestral(a, mo, fam, *ml, values, res, be);
    if (mo.joint_given) write_ml_joint(a, mo, fam, *ml, values, res, be);
    if (mo.samples_given) write_ml_samples(a, mo, fam, *ml, values, res, be);
    if (mo.support_given) write_ml_support(a, mo, fam, *ml, values, res, be);
}
// --guidance (Penn et al. 2010, GUIDANCE: the guide tree as the source of alignment uncertainty): the final alignment's columns are
// resampled N times as --bootstrap resamples them, every replicate's BioNJ tree, midpoint rooted and written with exact branch
// lengths, is read back as `-t` reads a tree and used as the guide tree of a realignment of the family's sequences (forest passes
// over groups of replicates within --batch_cells), and Backend::msa_agreement counts per group how often the residue pairs of the
// alignment as written (start / stop columns re-inserted, ancestral rows left out) share a column in the replicates' alignments.
void doGuidance(const Alphabet &a, const DriverOptions &o, const Family &fam, const CSProfile *csprofile) {
    typedef std::chrono::steady_clock clk;
    const auto t0 = clk::now();
    Backend &be = default_backend();
    const GuidanceOpts &go = o.guidance;
    const uint32_t N = (uint32_t)go.n;
    const std::map<std::string, sequence_t> rows = sequence_rows(fam.result.aligned_sequences);
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
        std::vector<PhyTree *> unrooted = bootstrap_trees(a, rows, fam.model_factory.get(), N, go.seed);
        bootstrap_stats = kept;
        for (uint32_t r = 0; r < N; ++r) trees[r].reset(unrooted[r]);
        for (uint32_t r = 0; r < N; ++r) {
            trees[r].reset(midpointRoot(trees[r].release()));
            const std::string text = format_newick_exact(*trees[r]);
            if (!go.dump.empty()) {
                open_output(go.dump + "." + std::to_string(r) + ".nwk", "guidance dump") << text << std::endl;
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
            if (groups.empty() || sum + cells[r] > o.batch_cells) { groups.emplace_back(r, r); sum = 0; }
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
                ff[k].repeats = fam.repeats; ff[k].result = &res[k];
                cost[k] = (uint64_t)cells[grp.first + k] + 1u;
            }
            const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, be.workers());   // (as doBatch deals families)
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
            if (!go.dump.empty()) {   // the replicate's alignment as `-t <its tree>` writes it
                const uint32_t r = grp.first + (uint32_t)k;
                std::map<std::string, std::string> aligned;
                fam.finish_rows(a, res[k].aligned_sequences, aligned);
                std::ofstream out = open_output(go.dump + "." + std::to_string(r) + ".fa", "guidance dump");
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
    std::ofstream out = open_output(go.out, "guidance output"), rout;
    if (!go.residues.empty()) rout = open_output(go.residues, "guidance residue");
    guidance_write(G, names, where0.data(), go.seed, out, go.residues.empty() ? nullptr : &rout);
    guidance_stats.replicates += (int)N;
    guidance_stats.seconds += std::chrono::duration<double>(clk::now() - t0).count();
}

}  // namespace pgm
