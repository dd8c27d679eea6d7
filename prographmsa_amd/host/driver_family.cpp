// driver_family.cpp — one family's outputs, the estimate of its cost, and the loop of alignment and tree re-estimation that the solo
// run (a list of one family) and every chunk of a --batch run go through.
#include "driver_family.h"

#include <algorithm>
#include <chrono>
#include <cstdio>

namespace pgm {

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
// write_profile (profile.h:12-31; main.cpp:451-456): default stream formatting, 6 significant digits
void Family::write_profiles(const Alphabet &a, const std::string &path) const {
    std::ofstream pf(path.c_str());
    for (const auto &kv : result.profiles) {
        pf << '>' << kv.first << std::endl;
        for (int j = 0; j < a.DIM; ++j) {
            pf << value_name(a, j);
            for (index_t k = 0; k < kv.second.cols; ++k) pf << '\t' << kv.second.data[(size_t)j + (size_t)a.DIM * k];
            pf << std::endl;
        }
    }
}

// Estimated DP cells of one pass over a family: the sum over the internal nodes of its tree of (residues below the left child) x
// (residues below the right child) — an over-estimate that needs no alignment —, (N - 1) x (mean length)^2 before a tree exists.
double subtree_cells(const PhyTree &t, const std::map<std::string, sequence_t> &seqs, double &cells) {
    if (t.isLeaf()) { auto it = seqs.find(t.getName()); return it == seqs.end() ? 0.0 : (double)it->second.size(); }
    std::vector<double> below;
    double sum = 0;
    for (index_t c = 0; c < t.n_children(); ++c) { below.push_back(subtree_cells(t[(int)c], seqs, cells)); sum += below.back(); }
    if (below.size() == 2) cells += below[0] * below[1];
    return sum;
}
double estimate_cells(const Family &fam) {
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
        ff[k].repeats = act[k]->repeats; ff[k].result = &act[k]->result; ff[k].worker = act[k]->worker;
    }
    progressive_alignment_forest(a, ff, csprofile);
    for (size_t k = 0; k < act.size(); ++k) if (!ff[k].error.empty()) act[k]->failure = ff[k].error;
}
// A tree for every family of `act`, from its sequences or from its alignment.
static void trees_for(const Alphabet &a, const std::vector<Family *> &act, bool prealigned, bool solo) {
    if (solo) {
        for (Family *f : act) {
            const auto t0 = std::chrono::steady_clock::now();
            try { f->tree = TreeNJ(a, prealigned ? f->result.aligned_sequences : f->seqs2, f->model_factory.get(), prealigned, f->topo); }
            catch (std::exception &e) { f->failure = e.what(); continue; }
            if (prealigned && host_switches().profile) fprintf(stderr, "guide tree from the alignment: %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        return;
    }
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
std::vector<Family *> alive(const std::vector<Family *> &v) {
    std::vector<Family *> out;
    for (Family *f : v) if (f->failure.empty()) out.push_back(f);
    return out;
}
void initial_trees(const Alphabet &a, const std::vector<Family *> &chunk, bool solo) {
    std::vector<Family *> need;
    for (Family *f : chunk) if (!f->tree) need.push_back(f);
    if (!need.empty()) trees_for(a, need, false, solo);
}

// The families of a chunk through the stages of doAlign in lock-step: every device stage once for all of them.
void align_rounds(const Alphabet &a, const std::vector<Family *> &chunk, const CSProfile *csprofile, bool solo) {
    // rounds of alignment followed by a tree from the alignment (main.cpp:404-430), per family as far as its own loop goes
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
        if (!go_on.empty()) trees_for(a, go_on, true, solo);
        for (Family *f : alive(go_on)) f->old_result = f->result;
    }
    // the final alignment (main.cpp:433-440): with -r (refused with --batch) the guide tree rerooted on the branch of the lowest gap
    // parsimony; with -T there is none, nor for a solo run that has failed
    if (cmdlineopts.onlytree_flag || (solo && alive(chunk).empty())) return;
    if (cmdlineopts.reroot_flag)
        for (Family *f : alive(chunk)) f->result = progressive_alignment_find_root(a, f->seqs2, *f->tree, *f->model_factory, f->repeats);
    else forest_pass(a, alive(chunk), csprofile);
}

}  // namespace pgm
