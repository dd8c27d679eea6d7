// progressive_internal.h — what the plain pass (progressive.cpp), the root search (root_search.cpp) and the repeat annotation
// (repeats.cpp) share and nobody else needs: the node of a pass, the environment of a level of merges, the leaf builders.
#pragma once
#include "pgm_host.h"

#include <chrono>

namespace pgm {

struct Node {
    std::string tr_note;   // -R: "TR indels at (...): n" of this internal node
    const PhyTree *tree;   // the guide-tree node (a merge of the root search's DAG has none; its leaves have theirs)
    int fam = 0;           // the family (tree of a forest pass) the node belongs to: LevelEnv::fams
    int child[2] = {-1, -1};
    double len[2] = {0, 0}, sup[2] = {1, 1};   // length and support of the branches to the two children
    int height = 0;
    int refs = 0;          // merges that still read this result (the root search's DAG: up to three)
    ProgressiveAlignmentResult res;
    std::vector<index_t> map[2];   // the root search: anc.mapping1 / mapping2 of the merge (rows are not carried through the DAG)
};
// what differs between the families of a forest pass: the models (-F estimates the frequencies per family) and the repeats
struct FamEnv {
    const ModelFactory *model_factory;
    const std::map<std::string, std::vector<repeat_t>> *repeats;
    bool with_repeats() const { return repeats && !repeats->empty(); }
};
// what a level of merges needs besides the nodes: the plain pass and the root search's DAG run the same code
struct LevelEnv {
    const Alphabet &a;
    std::vector<FamEnv> fams;   // indexed by Node::fam (one entry for a single tree and for the root search)
    bool resident_pass;
    bool earlyref;   // early refinement of every merged node (the plain pass with --early_refinement)
    bool dag;        // the root search: merges keep their mappings instead of extending rows; children released by reference count
    std::chrono::steady_clock::time_point tl0;
};

// align_progressive_results (ProgressiveAlignment.h:413-476) of every node of `level` (their children are done) in one batch
void run_level(const LevelEnv &env, std::vector<Node> &nodes, std::vector<int> &owner, const std::vector<int> &level, int h);

// extend_alignment (ProgressiveAlignment.h:245-264): the rows of a child as rows of the merged graph of n nodes
// `spread`: the rows are filled on the host threads (the few nodes near the root carry hundreds of rows each)
void extend_rows(const Alphabet &a, std::map<std::string, sequence_t> &out, index_t n, const std::vector<index_t> &mapping,
                 const std::map<std::string, sequence_t> &aligned_sequences, bool spread);

// The result of a leaf before any merge (ProgressiveAlignment.cpp:17-46): score 0, no TR indels, not a context profile; its own
// row under `row_name` (the root search carries no rows: nullptr); the graph of `seq` with its one-hot profiles on the host, or
// without them (OnDevice: upload_onehot_leaves builds them), or none yet (the context-profile leaves get theirs later).
enum class LeafGraph { OnHost, OnDevice, None };
void init_leaf(const Alphabet &a, ProgressiveAlignmentResult &res, const sequence_t &seq, LeafGraph graph, const std::string *row_name);
// the one-hot profiles of the OnDevice leaves `leaves` (seq_of[v]: the sequence of leaf nodes[v]) built on device context `worker`
void upload_onehot_leaves(const Alphabet &a, std::vector<Node> &nodes, const std::vector<int> &leaves, const std::vector<const sequence_t *> &seq_of, int worker);

// repeats.cpp: the annotation of leaf `name`; the repeat units of a child in the merged graph
void attach_repeats(ProgressiveAlignmentResult &res, const std::string &name, const std::map<std::string, std::vector<repeat_t>> &repeats);
void extend_tr_homologies(ProgressiveAlignmentResult &result, const std::vector<index_t> &mapping, const std::vector<std::vector<int>> &tr_homologies,
                          const std::vector<std::string> &tr_source);

}  // namespace pgm
