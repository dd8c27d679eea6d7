// driver_family.h — the state of one family in the driver and the loop every run walks it through (driver_family.cpp).
#pragma once
#include "pgm_host.h"

#include <fstream>

namespace pgm {

// What doAlign keeps for one family (main.cpp:332-482): the solo run is this state for one family, `--batch` walks the states of
// a chunk of families through the same stages together.
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
    const std::map<std::string, std::vector<repeat_t>> *repeats = nullptr;   // --read_repeats (solo only)
    ProgressiveAlignmentResult result, old_result;
    bool done = false;   // converged: takes no further part in the iterations
    std::string failure;   // the message the run of this family ends with (solo: rethrown; --batch: reported, the others go on)
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
    void write_profiles(const Alphabet &a, const std::string &path) const;   // --profile_out
};

// Estimated DP cells of one pass: over a tree, and over a family (before it has a tree: from its sequences alone)
double subtree_cells(const PhyTree &t, const std::map<std::string, sequence_t> &seqs, double &cells);
double estimate_cells(const Family &fam);
std::vector<Family *> alive(const std::vector<Family *> &v);   // the families without a failure
// A run in two parts (the solo run times them apart): a guide tree for every family that has none, then the rounds of alignment
// and tree re-estimation and the final alignment.  `solo`: the trees come from TreeNJ (the pair counts spread over every device
// context), not from TreeNJ_multi.  A family that cannot go on keeps the message in `failure` and takes no further part.
void initial_trees(const Alphabet &a, const std::vector<Family *> &chunk, bool solo);
void align_rounds(const Alphabet &a, const std::vector<Family *> &chunk, const CSProfile *csprofile, bool solo);

}  // namespace pgm
