// progressive.cpp — progressive alignment driver (reference src/ProgressiveAlignment.{h,cpp}).
//
// The reference recurses strictly sequentially (ProgressiveAlignment.cpp:50-51).  The results of
// sibling subtrees are independent, so this driver walks the tree level by level ("height" = longest
// path to a leaf) and hands every ready internal node of a level to the backend in ONE batched
// alignGraphs call; the per-node host work (CleanedGraph, mergeGraphs, extend_alignment) runs on a
// few host threads.  The values produced per node are those of the reference's recursion.
#include "pgm_host.h"
#include "../csrc/pgm_pool.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <thread>

namespace pgm {

// extend_alignment (ProgressiveAlignment.h:245-264): the rows of a child as rows of the merged graph of n nodes
void parallel_for(size_t n, const std::function<void(size_t)> &fn);
// `spread`: the rows are filled on the host threads (the few nodes near the root carry hundreds of rows each)
static void extend_rows(const Alphabet &a, std::map<std::string, sequence_t> &out, index_t n, const std::vector<index_t> &mapping,
                        const std::map<std::string, sequence_t> &aligned_sequences, bool spread) {
    std::vector<std::pair<const sequence_t *, sequence_t *>> rows;
    rows.reserve(aligned_sequences.size());
    for (const auto &kv : aligned_sequences) rows.emplace_back(&kv.second, &out[kv.first]);
    auto fill = [&](size_t r) {
        sequence_t extended(n - 2, a.unknown());
        const sequence_t &original = *rows[r].first;
        index_t k = 0;
        for (index_t j = 1; j < n - 1; ++j) {
            if (mapping[j] != (index_t)-1) extended[j - 1] = original[k++];
            else extended[j - 1] = a.gap();
        }
        *rows[r].second = std::move(extended);
    };
    if (spread && rows.size() >= 64) parallel_for(rows.size(), fill);
    else for (size_t r = 0; r < rows.size(); ++r) fill(r);
}
static void extend_alignment(const Alphabet &a, ProgressiveAlignmentResult &result, const std::vector<index_t> &mapping,
                             const std::map<std::string, sequence_t> &aligned_sequences, bool spread) {
    extend_rows(a, result.aligned_sequences, result.graph.size(), mapping, aligned_sequences, spread);
}

// ancestral sequences and profiles (--ancestral_seqs; ProgressiveAlignment.h:289-411)
static std::string create_ancestral_seq_name(const std::map<std::string, sequence_t> &aligned_seqs) {
    std::vector<std::string> leaves;
    for (const auto &kv : aligned_seqs) if (kv.first[0] != '(') leaves.push_back(kv.first);
    std::sort(leaves.begin(), leaves.end());
    std::string s = "(";
    for (size_t i = 0; i < leaves.size(); ++i) { if (i) s += ","; s += leaves[i]; }
    return s + ")";
}
static int8_t symbol_of(const Alphabet &a, int j) {   // ALPHABET(j): the symbol whose value() is j
    static const char *aa = "ACDEFGHIKLMNPQRSTVWY";
    if (a.kind == ALPHA_AA) return sequenceFromString(a, std::string(1, aa[j]))[0];
    static const char nt[] = "TCAG";   // the 61 sense codons in TCAG order (Alphabet.cpp)
    if (a.kind == ALPHA_DNA) return j < 4 ? (int8_t)nt[j] : a.unknown();   // dna_inv_translation_table
    int k = -1;
    for (int c = 0; c < 64; ++c) {
        const std::string cod = {nt[c >> 4], nt[(c >> 2) & 3], nt[c & 3]};
        if (cod == "TAA" || cod == "TAG" || cod == "TGA") continue;
        if (++k == j) return sequenceFromString(a, cod)[0];
    }
    return a.unknown();
}
// the sequence and the profile of `src`'s nodes as seen from the (new) graph of `result`: node i of the result shows column
// (col .* pi) of source node mapping[i] if it is a matched node, a gap otherwise.  prelim: src = result.graph itself.
static void ancestral_seq(const Alphabet &a, ProgressiveAlignmentResult &result, const std::string &anc_name, const Graph &src, const std::vector<index_t> *mapping,
                          const std::vector<bool> &matched, const Model &model) {
    const index_t n = result.graph.size();
    const int D = a.DIM;
    sequence_t extended(n - 2, a.unknown());
    Profile prof;
    prof.dim = D;
    std::vector<double> col((size_t)D);
    for (index_t i = 1; i < n - 1; ++i) {
        const bool on = matched[i] && (!mapping || (*mapping)[i] != (index_t)-1);
        if (!on) { extended[i - 1] = a.gap(); continue; }
        const double *g = src.col(mapping ? (*mapping)[i] : i);
        int best = 0;
        double sum = 0;
        for (int k = 0; k < D; ++k) { col[(size_t)k] = g[k] * model.pi[(size_t)k]; if (col[(size_t)k] > col[(size_t)best]) best = k; }   // maxCoeff: the first maximum
        extended[i - 1] = symbol_of(a, best);
        for (int k = 0; k < D; ++k) sum += col[(size_t)k];
        for (int k = 0; k < D; ++k) prof.data.push_back(col[(size_t)k] / sum);
        ++prof.cols;
    }
    result.aligned_sequences[anc_name] = extended;
    result.profiles[anc_name] = std::move(prof);
}

void parallel_for(size_t n, const std::function<void(size_t)> &fn) {
    static unsigned nt = []() {
        unsigned v = std::thread::hardware_concurrency();
        if (const char *e = getenv("PGM_HOST_THREADS")) v = (unsigned)atoi(e);
        return std::max(1u, std::min(v, 16u));
    }();
    static pgm_pool::Pool pool(nt);   // persistent: a level has half a dozen sections of a millisecond or two
    const std::string err = pool.run(n, nt, fn);
    if (!err.empty()) throw pgm_exception(err);
}

namespace {
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
struct Pending {  // state of one align_progressive_results call between its two halves
    Model model, model1, model2;
    std::unique_ptr<CleanedGraph> cg1, cg2;
};
}  // namespace

static int collect(const PhyTree &t, std::vector<Node> &nodes) {
    if (!t.isLeaf() && t.n_children() != 2) error("only bifurcating trees allowed");
    int c0 = -1, c1 = -1;
    if (!t.isLeaf()) {
        c0 = collect(t[0], nodes);
        c1 = collect(t[1], nodes);
    }
    Node n;
    n.tree = &t;
    n.child[0] = c0;
    n.child[1] = c1;
    if (!t.isLeaf())
        for (int i = 0; i < 2; ++i) { n.len[i] = t[i].getBranchLength(); n.sup[i] = t[i].getBranchSupport(); }
    n.height = t.isLeaf() ? 0 : 1 + std::max(nodes[c0].height, nodes[c1].height);
    nodes.push_back(std::move(n));
    return (int)nodes.size() - 1;
}

// extend_tr_homologies (ProgressiveAlignment.h:266-287)
static void extend_tr_homologies(ProgressiveAlignmentResult &result, const std::vector<index_t> &mapping, const std::vector<std::vector<int>> &tr_homologies,
                                 const std::vector<std::string> &tr_source) {
    const index_t n = result.graph.size();
    for (size_t r = 0; r < tr_homologies.size(); ++r) {
        std::vector<int> extended(n - 2, -1);
        const std::vector<int> &original = tr_homologies[r];
        index_t k = 0;
        for (index_t j = 1; j < n - 1; ++j) extended[j - 1] = mapping[j] != (index_t)-1 ? original[k++] : -1;
        result.tr_homologies.push_back(extended);
        result.tr_source.push_back(tr_source[r]);
    }
}

// --read_repeats: the T-REKS report (RepeatDetectionTReks.cpp:62-151).  Per sequence ('>' line) any number of repeats: a header
// line "Length: ... from S to E ..." (S 1-based), then the aligned repeat units, one per line, up to a line of asterisks; '-',
// blanks and tabs are gaps; the residues of the units must spell the sequence from position S on.
static std::string strip_ws(const std::string &s) {
    size_t b = 0, e = s.size();
    while (b < e && isspace((unsigned char)s[b])) ++b;
    while (e > b && isspace((unsigned char)s[e - 1])) --e;
    return s.substr(b, e - b);
}
std::map<std::string, std::vector<repeat_t>> read_repeats(const Alphabet &a, const std::string &filename, const std::map<std::string, sequence_t> &seqs) {
    std::map<std::string, std::string> seqs2;
    for (const auto &kv : seqs) seqs2[kv.first] = stringFromSequence(a, kv.second);
    std::ifstream in(filename.c_str());
    std::map<std::string, std::vector<repeat_t>> map;
    index_t n_sequences = 0, n_repeats = 0;
    std::string name, line;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') { name = strip_ws(line.substr(1)); ++n_sequences; }
        else if (line.compare(0, 7, "Length:") == 0) {
            const size_t from = line.find("from");
            if (from == line.npos) throw pgm_exception("format error (from)");
            const size_t to = line.find("to", from);
            if (to == line.npos) throw pgm_exception("format error (to)");
            repeat_t repeat;
            ++n_repeats;
            long start = 0;
            { std::stringstream ss; ss << line.substr(from + 4, to - from - 4); ss >> start; if (!ss || start <= 0) throw pgm_exception("format error (number)"); }
            repeat.start = (index_t)(start - 1);
            auto orig_entry = seqs2.find(name);
            if (orig_entry == seqs2.end()) throw pgm_exception("unknown sequence name: " + name);
            size_t orig = repeat.start;
            repeat.len = (index_t)-1;
            while (std::getline(in, line)) {
                line = strip_ws(line);
                if (line.compare(0, 22, "**********************") == 0) break;
                for (char &c : line) if (c == '-' || c == ' ' || c == '\n' || c == '\t' || c == '\r') c = '_';
                if (repeat.len != (index_t)-1 && line.size() != repeat.len) throw pgm_exception("repeat unit lengths differ");
                repeat.len = (index_t)line.size();
                for (index_t i = 0; i < repeat.len; ++i)
                    if (line[i] != '_') {
                        repeat.tr_hom.push_back((int)i);
                        if (orig >= orig_entry->second.size() || orig_entry->second[orig] != line[i]) throw pgm_exception("character mismatch in repeat of \"" + name + "\"");
                        ++orig;
                    }
            }
            map[name].push_back(repeat);
        }
    }
    std::cerr << "found " << n_repeats << " repeats in " << n_sequences << " sequences" << std::endl;
    return map;
}

// tandem-repeat annotation of the leaves (ProgressiveAlignment.cpp:30-38)
static void attach_repeats(std::vector<Node> &nodes, const std::vector<int> &leaves, const std::map<std::string, std::vector<repeat_t>> *repeats) {
    if (!repeats || repeats->empty()) return;
    for (int li : leaves) {
        Node &nd = nodes[li];
        auto it2 = repeats->find(nd.tree->getName());
        if (it2 == repeats->end()) continue;
        for (const repeat_t &rep : it2->second) {
            std::vector<int> tr_hom(nd.res.graph.size(), -1);
            if ((size_t)rep.start + 1 + rep.tr_hom.size() > tr_hom.size()) error("repeat beyond the end of sequence %s", nd.tree->getName().c_str());
            std::copy(rep.tr_hom.begin(), rep.tr_hom.end(), tr_hom.begin() + rep.start + 1);
            nd.res.tr_homologies.push_back(tr_hom);
            nd.res.tr_source.push_back(nd.tree->getName());
        }
        nd.res.graph.addRepeats(nd.res.tr_homologies);
    }
}

// A resident pass on several device contexts: the guide tree is cut into subtrees — the most expensive subtree of the cut is replaced
// by its two children until there are three per worker (or only leaves are left) —, the subtrees are dealt to the workers by cost
// (longest first to the least loaded: farm_shards), and every node of a subtree belongs to its worker: leaves are built there, jobs
// run there, merged profiles stay there.  A node above the cut belongs to the worker of its more expensive child; the other child's
// profiles are copied over once (Backend::resident_import).  cost(node) = sum over the internal nodes below of the product of the
// children's mean leaf lengths: the DP cells, near enough.  `nodes` is in post-order (children before parents).
static std::vector<int> assign_owners(const std::vector<Node> &nodes, int root, int nworkers, const std::vector<double> &leaf_len) {
    const size_t n = nodes.size();
    std::vector<double> cost(n, 0.0), len_sum(n, 0.0), nleaf(n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        if (nodes[i].child[0] < 0) { len_sum[i] = leaf_len[i]; nleaf[i] = 1.0; continue; }
        const int c0 = nodes[i].child[0], c1 = nodes[i].child[1];
        len_sum[i] = len_sum[c0] + len_sum[c1]; nleaf[i] = nleaf[c0] + nleaf[c1];
        cost[i] = cost[c0] + cost[c1] + (len_sum[c0] / nleaf[c0]) * (len_sum[c1] / nleaf[c1]);
    }
    std::vector<int> owner(n, 0);
    if (nworkers <= 1) return owner;
    std::vector<int> cut{root};
    std::vector<char> above(n, 0);
    while (cut.size() < 3 * (size_t)nworkers) {
        int pick = -1;
        for (size_t k = 0; k < cut.size(); ++k)
            if (nodes[cut[k]].child[0] >= 0 && (pick < 0 || cost[cut[k]] > cost[cut[(size_t)pick]])) pick = (int)k;
        if (pick < 0) break;
        const int v = cut[(size_t)pick];
        above[v] = 1;
        cut[(size_t)pick] = nodes[v].child[0];
        cut.push_back(nodes[v].child[1]);
    }
    std::vector<uint64_t> c64(cut.size());
    for (size_t k = 0; k < cut.size(); ++k) c64[k] = (uint64_t)cost[cut[k]] + 1u;
    const std::vector<std::vector<uint32_t>> shards = farm_shards(c64, nworkers);
    for (size_t w = 0; w < shards.size(); ++w)
        for (uint32_t k : shards[w]) {
            std::vector<int> stack{cut[k]};
            while (!stack.empty()) {
                const int v = stack.back(); stack.pop_back();
                owner[v] = (int)w;
                if (nodes[v].child[0] >= 0) { stack.push_back(nodes[v].child[0]); stack.push_back(nodes[v].child[1]); }
            }
        }
    for (size_t i = 0; i < n; ++i)   // post-order: the children of a node above the cut have their owners
        if (above[i]) owner[i] = cost[nodes[i].child[0]] + nleaf[nodes[i].child[0]] >= cost[nodes[i].child[1]] + nleaf[nodes[i].child[1]] ? owner[nodes[i].child[0]] : owner[nodes[i].child[1]];
    return owner;
}

// earlyRefinement (ProgressiveAlignment.h:114-243) of the nodes of one level, right after their alignment: the node's graph is
// aligned once more with the graph of every grandchild (of a leaf child: with the leaf) — the second call site of alignGraphs
// (:170), on the graphs as they are, not cleaned — and rebuilt from those alignments one descendant at a time
// (mergeGraphsIncremental); nodes no descendant maps to are dropped.  The 2-4 alignments of a node read only the node's old graph,
// so the whole level goes to the backend as ONE batch; the merges are per node, in the reference's order.
namespace {
// what differs between the families of a forest pass: the models (-F estimates the frequencies per family) and the repeats
struct FamEnv {
    const ModelFactory *model_factory;
    const std::map<std::string, std::vector<repeat_t>> *repeats;
    bool with_repeats() const { return repeats && !repeats->empty(); }
};
}  // namespace

static void early_refinement(const Alphabet &a, std::vector<Node> &nodes, const std::vector<int> &level, const std::vector<FamEnv> &fams) {
    const index_t NONE = (index_t)-1;
    struct Desc { int node; double distance, gap_distance; };
    std::vector<std::vector<Desc>> desc(level.size());
    std::vector<Model> models;
    std::vector<std::pair<size_t, size_t>> job_of;   // (position in the level, descendant)
    auto is_leaf = [&](int v) { return nodes[(size_t)v].child[0] < 0; };
    for (size_t k = 0; k < level.size(); ++k) {
        const Node &nd = nodes[(size_t)level[k]];
        if (is_leaf(nd.child[0]) && is_leaf(nd.child[1])) continue;   // (:124-125: nothing to refine)
        for (int i = 0; i < 2; ++i) {
            const int c = nd.child[i];
            const PhyTree &ct = *nodes[(size_t)c].tree;
            if (is_leaf(c)) {
                desc[k].push_back(Desc{c, nodes[(size_t)c].res.is_csprofile ? 0.0 : ct.getBranchLength(), ct.getBranchLength()});
            } else {
                for (int j = 0; j < 2; ++j) {
                    const int gc = nodes[(size_t)c].child[j];
                    const double bl = nodes[(size_t)gc].tree->getBranchLength();
                    desc[k].push_back(Desc{gc, ct.getBranchLength() + (nodes[(size_t)gc].res.is_csprofile ? 0.0 : bl), ct.getBranchLength() + bl});
                }
            }
        }
        const ModelFactory &model_factory = *fams[(size_t)nd.fam].model_factory;
        for (size_t i = 0; i < desc[k].size(); ++i) { models.push_back(model_factory.getModel(desc[k][i].distance, desc[k][i].gap_distance)); job_of.emplace_back(k, i); }
    }
    if (job_of.empty()) return;
    std::vector<const Graph *> g1(job_of.size()), g2(job_of.size());
    std::vector<const Model *> mm(job_of.size());
    for (size_t q = 0; q < job_of.size(); ++q) {
        g1[q] = &nodes[(size_t)level[job_of[q].first]].res.graph;
        g2[q] = &nodes[(size_t)desc[job_of[q].first][job_of[q].second].node].res.graph;
        mm[q] = &models[q];
    }
    std::vector<AlignmentResult> ar = alignGraphsBatch(g1, g2, mm, {}, {});
    std::vector<size_t> first_job(level.size(), 0);
    for (size_t q = job_of.size(); q-- > 0;) first_job[job_of[q].first] = q;
    parallel_for(level.size(), [&](size_t k) {
        const size_t nres = desc[k].size();
        if (nres == 0) return;
        Node &nd = nodes[(size_t)level[k]];
        const ProgressiveAlignmentResult &old_result = nd.res;
        Graph anc_graph = old_result.graph;
        anc_graph.reset();
        std::vector<index_t> anc_mapping(anc_graph.size());
        for (index_t i = 0; i < anc_graph.size(); ++i) anc_mapping[i] = i;
        std::vector<std::vector<index_t>> mappings(nres);
        for (size_t i = 0; i < nres; ++i) {
            AlignmentResult &al = ar[first_job[k] + i];
            const Graph &dg = nodes[(size_t)desc[k][i].node].res.graph;
            for (index_t &m : al.mapping1) if (m != NONE) m = anc_mapping[m];
            AncestralResult anc = mergeGraphsIncremental(anc_graph, dg, al.mapping1, al.mapping2, models[first_job[k] + i]);
            anc_graph = anc.graph;
            mappings[i] = anc.mapping2;
            /* the old graph's nodes inside the new ancestral graph, which is a superset (:180-188) */
            std::vector<index_t> inv(anc_graph.size(), (index_t)-2);
            for (index_t j = 0; j < anc.mapping1.size(); ++j) if (anc.mapping1[j] != NONE) inv[anc.mapping1[j]] = j;
            for (index_t &m : anc_mapping) m = inv[m];
            for (size_t j = 0; j < i; ++j) {   // the earlier descendants' mappings follow (:190-198)
                std::vector<index_t> nm(anc_graph.size());
                for (index_t v = 0; v < anc_graph.size(); ++v) nm[v] = anc.mapping1[v] != NONE ? mappings[j][anc.mapping1[v]] : NONE;
                mappings[j].swap(nm);
            }
        }
        /* remove the nodes no descendant uses (:201-228) */
        auto used = [&](index_t v) { for (size_t j = 0; j < nres; ++j) if (mappings[j][v] != NONE) return true; return false; };
        for (index_t i = 0; i < anc_graph.size(); ++i) {
            if (used(i)) continue;
            for (index_t j = i + 1; j < anc_graph.size(); ++j)
                if (used(j)) {
                    anc_graph.rmNodes(i, j - i);
                    for (size_t q = 0; q < nres; ++q) mappings[q].erase(mappings[q].begin() + i, mappings[q].begin() + j);
                    --i;
                    break;
                }
        }
        ProgressiveAlignmentResult result;
        result.score = old_result.score;
        result.is_csprofile = false;
        result.n_tr_indels = old_result.n_tr_indels;
        result.graph = anc_graph;
        for (size_t i = 0; i < nres; ++i) {
            const ProgressiveAlignmentResult &dr = nodes[(size_t)desc[k][i].node].res;
            extend_alignment(a, result, mappings[i], dr.aligned_sequences, false);
            extend_tr_homologies(result, mappings[i], dr.tr_homologies, dr.tr_source);
        }
        if (fams[(size_t)nd.fam].with_repeats()) result.graph.addRepeats(result.tr_homologies);
        nd.res = std::move(result);
    });
}

namespace {
// what a level of merges needs besides the nodes: the plain pass and the root search's DAG run the same code
struct LevelEnv {
    const Alphabet &a;
    std::vector<FamEnv> fams;   // indexed by Node::fam (one entry for a single tree and for the root search)
    bool resident_pass;
    bool earlyref;   // early refinement of every merged node (the plain pass with --early_refinement)
    bool dag;        // the root search: merges keep their mappings instead of extending rows; children released by reference count
    std::chrono::steady_clock::time_point tl0;
};
}  // namespace

// align_progressive_results (ProgressiveAlignment.h:413-476) of every node of `level` (their children are done) in one batch
static void run_level(const LevelEnv &env, std::vector<Node> &nodes, std::vector<int> &owner, const std::vector<int> &level, int h) {
    const Alphabet &a = env.a;
    const bool resident_pass = env.resident_pass;
    const auto tl0 = env.tl0;
    const size_t L = level.size();
    std::vector<Pending> pend(L);
    const auto tp0 = std::chrono::steady_clock::now();
    if (resident_pass)   // children of a node above the cut of the subtrees: the profiles of the one on another worker are copied over
        for (size_t k = 0; k < L; ++k) {
            const Node &nd = nodes[level[k]];
            for (int c = 0; c < 2; ++c) {
                const int ch = nd.child[c];
                Graph &g = nodes[ch].res.graph;
                if (owner[(size_t)ch] == owner[(size_t)level[k]] || !g.devSites()) continue;
                const double *there = default_backend().resident_import(owner[(size_t)level[k]], owner[(size_t)ch], g.devSites(), (size_t)a.DIM * g.size());
                if (!there) error("the backend could not copy resident profiles between its workers");
                g.setDevSites(there);
                owner[(size_t)ch] = owner[(size_t)level[k]];
                ++default_backend().resident_imports;
            }
        }
    parallel_for(L, [&](size_t k) {
        Node &nd = nodes[level[k]];
        const ProgressiveAlignmentResult &r1 = nodes[nd.child[0]].res, &r2 = nodes[nd.child[1]].res;
        double distance1 = nd.len[0], distance2 = nd.len[1];
        double gap_distance1 = distance1, gap_distance2 = distance2;
        if (r1.is_csprofile) distance1 = 0;
        if (r2.is_csprofile) distance2 = 0;
        Pending &p = pend[k];
        const ModelFactory &model_factory = *env.fams[(size_t)nd.fam].model_factory;
        p.model = model_factory.getModel(distance1 + distance2, gap_distance1 + gap_distance2);
        p.model1 = model_factory.getModel(distance1, gap_distance1);
        p.model2 = model_factory.getModel(distance2, gap_distance2);
        p.cg1.reset(new CleanedGraph(r1.graph));
        p.cg2.reset(new CleanedGraph(r2.graph));
    });
    const auto tp1 = std::chrono::steady_clock::now();
    std::vector<const Graph *> g1(L), g2(L);
    std::vector<const Model *> mm(L);
    for (size_t k = 0; k < L; ++k) { g1[k] = pend[k].cg1.get(); g2[k] = pend[k].cg2.get(); mm[k] = &pend[k].model; }
    // graphs merged on the device one level below: their profiles never left it (gathered there through the cleaned graphs' node maps)
    std::vector<pgm_site_ref> rs1, rs2;
    {
        bool any = false;
        for (size_t k = 0; k < L; ++k) any = any || pend[k].cg1->devSites() || pend[k].cg2->devSites();
        if (any) {
            rs1.assign(L, pgm_site_ref{nullptr, nullptr, 0u}); rs2.assign(L, pgm_site_ref{nullptr, nullptr, 0u});
            for (size_t k = 0; k < L; ++k) {
                if (pend[k].cg1->devSites()) rs1[k] = pgm_site_ref{pend[k].cg1->devSites(), pend[k].cg1->nodeMap(), (uint32_t)pend[k].cg1->originalSize()};
                if (pend[k].cg2->devSites()) rs2[k] = pgm_site_ref{pend[k].cg2->devSites(), pend[k].cg2->nodeMap(), (uint32_t)pend[k].cg2->originalSize()};
            }
        }
    }
    std::vector<int> worker_of(L, 0);
    for (size_t k = 0; k < L; ++k) worker_of[k] = owner[(size_t)level[k]];
    std::vector<AlignmentResult> ar = alignGraphsBatch(g1, g2, mm, rs1, rs2, resident_pass && default_backend().workers() > 1 ? &worker_of : nullptr);
    const auto tp2 = std::chrono::steady_clock::now();
    // mergeGraphs of the whole level: plans on host threads, the node profiles (P g products, L2 normalisation: the
    // arithmetic of the merge) in ONE device batch, then edges / Graph / extend_alignment on host threads again
    std::vector<MergePlan> plans(L);
    std::vector<std::vector<double>> profiles(L);
    // The merged profiles stay on the device when nothing on the host reads them: one device context, no --profile_out /
    // --ancestral_seqs, no job dump (Backend::resident; PGM_NO_RESIDENT=1 keeps the round trip)
    const bool resident = resident_pass;
    std::vector<const double *> dev_profiles(L, nullptr);
    parallel_for(L, [&](size_t k) {
        Node &nd = nodes[level[k]];
        Pending &p = pend[k];
        p.cg1->uncleanMapping(ar[k].mapping1);
        p.cg2->uncleanMapping(ar[k].mapping2);
        plans[k] = planMerge(nodes[nd.child[0]].res.graph, nodes[nd.child[1]].res.graph, ar[k].mapping1, ar[k].mapping2);
        if (!resident) profiles[k].assign((size_t)a.DIM * plans[k].mapping1.size(), 0.0);
    });
    const auto tq0 = std::chrono::steady_clock::now();
    bool on_device = false;
    // (a resident pass: the graphs below need the plans only, not the profiles — the device batch of the node profiles runs on a
    // thread of its own beside them)
    std::thread merge_thread;
    std::exception_ptr merge_error;
    std::vector<pgm_merge_job> mj(L);   // (filled before the thread starts: the graphs section below releases the children)
    bool all_on_device = true;
    if (!host_switches().host_merge)
        for (size_t k = 0; k < L; ++k) {
            Node &nd = nodes[level[k]];
            const Graph &ga = nodes[nd.child[0]].res.graph, &gb = nodes[nd.child[1]].res.graph;
            pgm_merge_job &j = mj[k];
            j.dim = (uint32_t)a.DIM; j.n1 = ga.size(); j.n2 = gb.size(); j.nnodes = (uint32_t)plans[k].mapping1.size();
            j.sites1 = ga.devSites() ? ga.devSites() : ga.col(0); j.sites2 = gb.devSites() ? gb.devSites() : gb.col(0);
            j.P1 = pend[k].model1.P.data(); j.P2 = pend[k].model2.P.data();
            j.k1 = plans[k].mapping1.data(); j.k2 = plans[k].mapping2.data(); j.g2_with_P1 = plans[k].g2_with_P1.data();
            j.profiles = resident ? nullptr : profiles[k].data();
            all_on_device = all_on_device && ga.devSites() && gb.devSites();
        }
    auto merge_on_device = [&]() {
    if (!host_switches().host_merge) {
        const auto tm0 = std::chrono::steady_clock::now();
        {
            // the merges of a level are independent: dealt to the device contexts by the size of the merged graph
            Backend &be = default_backend();
            std::vector<uint64_t> cost(L);
            for (size_t k = 0; k < L; ++k) cost[k] = mj[k].nnodes;
            const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, be.workers());
            if (resident && be.workers() > 1) {   // every merge where its children are: one batch per worker, concurrently
                std::vector<std::vector<uint32_t>> mine((size_t)be.workers());
                for (size_t k = 0; k < L; ++k) mine[(size_t)worker_of[k]].push_back((uint32_t)k);
                std::vector<char> ok(mine.size(), 1);
                farm_run(mine, [&](int w) {
                    const std::vector<uint32_t> &sh = mine[(size_t)w];
                    std::vector<pgm_merge_job> q(sh.size());
                    std::vector<const double *> dv(sh.size(), nullptr);
                    for (size_t k = 0; k < sh.size(); ++k) q[k] = mj[sh[k]];
                    ok[(size_t)w] = be.merge_profiles_batch_res((uint32_t)q.size(), q.data(), dv.data(), w) ? 1 : 0;
                    for (size_t k = 0; k < sh.size(); ++k) dev_profiles[sh[k]] = dv[k];
                });
                on_device = true;
                for (char c : ok) on_device = on_device && c;
                if (!on_device) error("the backend could not keep the merged profiles on the device");
            } else if (resident) {
                on_device = be.merge_profiles_batch_res((uint32_t)L, mj.data(), dev_profiles.data(), 0);
                if (!on_device) error("the backend could not keep the merged profiles on the device");
            } else if (shards.size() <= 1) {
                on_device = be.merge_profiles_batch((uint32_t)L, mj.data(), 0);
            } else {
                std::vector<char> ok(shards.size(), 0);
                farm_run(shards, [&](int w) {
                    const std::vector<uint32_t> &sh = shards[(size_t)w];
                    std::vector<pgm_merge_job> q(sh.size());
                    for (size_t k = 0; k < sh.size(); ++k) q[k] = mj[sh[k]];
                    ok[(size_t)w] = be.merge_profiles_batch((uint32_t)q.size(), q.data(), w) ? 1 : 0;
                });
                on_device = true;
                for (size_t w = 0; w < shards.size(); ++w) on_device = on_device && (ok[w] || shards[w].empty());
            }
        }
        default_backend().seconds_merge_profiles += std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count();
    }
    };
    if (resident && all_on_device && !host_switches().host_merge) merge_thread = std::thread([&]() { try { merge_on_device(); } catch (...) { merge_error = std::current_exception(); } });
    else merge_on_device();
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } merge_joiner{merge_thread};   // (also when the section below throws)
    const auto tq1 = std::chrono::steady_clock::now();
    std::atomic<long long> ns_merge(0), ns_extend(0);
    parallel_for(L, [&](size_t k) {
        const auto tk0 = std::chrono::steady_clock::now();
        Node &nd = nodes[level[k]];
        ProgressiveAlignmentResult &r1 = nodes[nd.child[0]].res, &r2 = nodes[nd.child[1]].res;
        Pending &p = pend[k];
        ProgressiveAlignmentResult &result = nd.res;
        result.score = ar[k].score;
        result.is_csprofile = false;
        result.n_tr_indels = ar[k].n_tr_indels + r1.n_tr_indels + r2.n_tr_indels;
        if (!resident && !on_device) mergeProfilesHost(r1.graph, r2.graph, p.model1, p.model2, plans[k], profiles[k]);
        AncestralResult anc = finishMerge(r1.graph, r2.graph, plans[k], resident ? nullptr : profiles[k].data(), nd.sup[0], nd.sup[1]);
        result.graph = anc.graph;
        const auto tk1 = std::chrono::steady_clock::now();
        if (!env.dag) {
            extend_alignment(a, result, anc.mapping1, r1.aligned_sequences, L == 1);
            extend_alignment(a, result, anc.mapping2, r2.aligned_sequences, L == 1);
        } else {
            nd.map[0] = anc.mapping1;
            nd.map[1] = anc.mapping2;
        }
        ns_merge += std::chrono::duration_cast<std::chrono::nanoseconds>(tk1 - tk0).count();
        ns_extend += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tk1).count();
        if (!r1.tr_homologies.empty() || !r2.tr_homologies.empty()) {   // ProgressiveAlignment.h:455-456, 468
            extend_tr_homologies(result, anc.mapping1, r1.tr_homologies, r1.tr_source);
            extend_tr_homologies(result, anc.mapping2, r2.tr_homologies, r2.tr_source);
        }
        if (!cmdlineopts.profile_file.empty() || cmdlineopts.ancestral_flag) {
            result.profiles.insert(r1.profiles.begin(), r1.profiles.end());
            result.profiles.insert(r2.profiles.begin(), r2.profiles.end());
        }
        if (cmdlineopts.ancestral_flag) {   // ProgressiveAlignment.h:458-466
            if (r1.aligned_sequences.size() > 1) ancestral_seq(a, result, create_ancestral_seq_name(r1.aligned_sequences), r1.graph, &anc.mapping1, anc.is_matched, p.model1);
            if (r2.aligned_sequences.size() > 1) ancestral_seq(a, result, create_ancestral_seq_name(r2.aligned_sequences), r2.graph, &anc.mapping2, anc.is_matched, p.model2);
            ancestral_seq(a, result, create_ancestral_seq_name(result.aligned_sequences), result.graph, nullptr, anc.is_matched, p.model);
        }
        if (cmdlineopts.repeats_flag && !env.dag) nd.tr_note = "TR indels at " + create_ancestral_seq_name(result.aligned_sequences) + ": " + std::to_string(ar[k].n_tr_indels);   // (:470-473)
        if (env.fams[(size_t)nd.fam].with_repeats()) result.graph.addRepeats(result.tr_homologies);   // (:468; with no annotation at all the merged graph has no repeat edges either way)
        // children are no longer needed (the reference copies them by value and drops them)
        if (!env.earlyref && !env.dag) {   // (the reference's alignment_cache, ProgressiveAlignment.h:107-109: the parent's refinement reads them again)
            r1 = ProgressiveAlignmentResult();
            r2 = ProgressiveAlignmentResult();
        }
        p.cg1.reset();
        p.cg2.reset();
        profiles[k] = std::vector<double>();
    });
    if (merge_thread.joinable()) {
        merge_thread.join();
        if (merge_error) std::rethrow_exception(merge_error);
    }
    if (resident) for (size_t k = 0; k < L; ++k) nodes[level[k]].res.graph.setDevSites(dev_profiles[k]);
    if (env.dag)   // a directed result of the root search is read by up to three merges, of any heights
        for (size_t k = 0; k < L; ++k)
            for (int c = 0; c < 2; ++c) {
                Node &ch = nodes[(size_t)nodes[level[k]].child[c]];
                if (--ch.refs == 0) ch.res = ProgressiveAlignmentResult();
            }
    if (env.earlyref) early_refinement(a, nodes, level, env.fams);
    const auto tp3 = std::chrono::steady_clock::now();
    if (host_switches().profile)
        fprintf(stderr, "[%.1f ms] level %d: %zu nodes, host pre %.1f ms, alignGraphsBatch %.1f ms, host post (merge, extend) %.1f ms\n",
                std::chrono::duration<double, std::milli>(tp3 - tl0).count(), h, L,
                std::chrono::duration<double, std::milli>(tp1 - tp0).count(), std::chrono::duration<double, std::milli>(tp2 - tp1).count(),
                std::chrono::duration<double, std::milli>(tp3 - tp2).count()),
        fprintf(stderr, "    post: plans %.1f ms, node profiles %.1f, edges / graphs / extend %.1f (summed over the nodes: graphs %.2f ms, extend_alignment %.2f)\n", std::chrono::duration<double, std::milli>(tq0 - tp2).count(),
                std::chrono::duration<double, std::milli>(tq1 - tq0).count(), std::chrono::duration<double, std::milli>(tp3 - tq1).count(), ns_merge.load() / 1e6, ns_extend.load() / 1e6);
}

BatchStats batch_stats;

// The pass over a forest: the nodes of every family's guide tree in one `nodes` vector, the leaf stage once for all of them, and one
// run_level per height over the nodes of that height of all trees.  A node reads its own children and its own family's models
// only, so what a family gets does not depend on the families it shares the pass with.  A family whose tree cannot be used (not
// bifurcating, a leaf that names no sequence) gets the solo pass's message in its `error` and takes no part.
void progressive_alignment_forest(const Alphabet &a, std::vector<ForestFamily> &families, const CSProfile *csprofile) {
    const auto tl0 = std::chrono::steady_clock::now();
    default_backend().resident_reset();   // (merged profiles a previous pass left on the device)
    ++batch_stats.passes;
    std::vector<Node> nodes;
    std::vector<FamEnv> fenv(families.size());
    std::vector<int> roots(families.size(), -1);
    int maxh = 0;
    const bool forest = families.size() > 1;
    for (size_t f = 0; f < families.size(); ++f) {
        ForestFamily &ff = families[f];
        fenv[f] = FamEnv{ff.model_factory, ff.repeats};
        ff.error.clear();
        const size_t first = nodes.size();
        try {
            const int root = collect(*ff.tree, nodes);
            for (size_t i = first; i < nodes.size(); ++i) {
                nodes[i].fam = (int)f;
                if (nodes[i].tree->isLeaf() && ff.sequences->find(nodes[i].tree->getName()) == ff.sequences->end()) error("unknown sequence name: %s", nodes[i].tree->getName().c_str());
            }
            roots[f] = root;
            maxh = std::max(maxh, nodes[(size_t)root].height);
        } catch (pgm_exception &e) {
            nodes.erase(nodes.begin() + (std::ptrdiff_t)first, nodes.end());
            ff.error = e.what();
        }
    }
    if (nodes.empty()) return;
    auto sequence_of = [&](int v) -> const sequence_t & { return families[(size_t)nodes[(size_t)v].fam].sequences->at(nodes[(size_t)v].tree->getName()); };

    // ---- leaves (ProgressiveAlignment.cpp:17-46) ----
    std::vector<int> leaves;
    for (size_t i = 0; i < nodes.size(); ++i)
        if (nodes[i].tree->isLeaf()) leaves.push_back((int)i);
    // A pass whose merged profiles stay on the device (see the level loop) builds its leaf graphs there too: the host keeps
    // their edges only (SequenceGraph's profile matrix is 160 bytes per residue: 41 MB for 256 x 1000, otherwise built here,
    // copied into the staging block and uploaded for the alignments, and once more for the merges)
    const bool resident_pass = default_backend().resident() && !host_switches().host_merge && cmdlineopts.profile_file.empty() && !cmdlineopts.ancestral_flag && !job_dump_active() &&
                               !cmdlineopts.earlyref_flag;   // (the incremental merges of an early refinement read the profiles on the host)
    const bool resident_leaves = resident_pass && !csprofile;
    // where the profiles of every node live (worker = device context): all 0 with one context
    std::vector<int> owner(nodes.size(), 0);
    if (forest && default_backend().workers() > 1) {   // a family never spans workers: nothing is copied between them
        for (size_t i = 0; i < nodes.size(); ++i) owner[i] = families[(size_t)nodes[i].fam].worker % default_backend().workers();
    } else if (resident_pass && default_backend().workers() > 1) {
        std::vector<double> leaf_len(nodes.size(), 0.0);
        for (int li : leaves) leaf_len[(size_t)li] = (double)sequence_of(li).size();
        owner = assign_owners(nodes, roots[(size_t)nodes[0].fam], default_backend().workers(), leaf_len);
    }
    default_backend().resident_pass = resident_pass;
    default_backend().resident_imports = 0;
    const auto tl1 = std::chrono::steady_clock::now();
    parallel_for(leaves.size(), [&](size_t k) {   // (independent leaves: a thousand SequenceGraphs are 50 ms on one thread)
        Node &nd = nodes[leaves[k]];
        auto it = families[(size_t)nd.fam].sequences->find(nd.tree->getName());
        nd.res.aligned_sequences[it->first] = it->second;
        nd.res.score = 0;
        nd.res.n_tr_indels = 0;
        nd.res.is_csprofile = false;
        if (resident_leaves) {
            nd.res.graph = Graph(a.DIM, (index_t)it->second.size() + 2, Graph::NoSites());
        } else if (!csprofile) {
            nd.res.graph = SequenceGraph(a, it->second);
            if (!cmdlineopts.profile_file.empty()) {   // result.profiles[name] = sites without START / END (ProgressiveAlignment.h:73)
                Profile &pf = nd.res.profiles[it->first];
                pf.dim = a.DIM; pf.cols = nd.res.graph.size() - 2;
                pf.data.assign(nd.res.graph.col(1), nd.res.graph.col(1) + (size_t)a.DIM * pf.cols);
            }
        }
    });
    const auto tl2 = std::chrono::steady_clock::now();
    if (resident_leaves && !leaves.empty()) {
        const int nw = default_backend().workers();
        for (int w = 0; w < nw; ++w) {   // every worker builds the leaves of its subtrees
            std::vector<int> mine;
            for (int li : leaves) if (owner[(size_t)li] == w) mine.push_back(li);
            if (mine.empty()) continue;
            std::vector<uint32_t> offs(mine.size() + 1, 0);
            std::vector<const sequence_t *> seqs(mine.size());
            for (size_t s = 0; s < mine.size(); ++s) {
                seqs[s] = &sequence_of(mine[s]);
                offs[s + 1] = offs[s] + (uint32_t)seqs[s]->size();
            }
            std::vector<int8_t> syms(offs[mine.size()]);
            parallel_for(mine.size(), [&](size_t s) {   // (a quarter of a million residues one push_back at a time: 1 ms of the leaf stage)
                int8_t *out = syms.data() + offs[s];
                for (int8_t c : *seqs[s]) *out++ = a.isValid(c) ? (int8_t)a.value(c) : (int8_t)-1;
            });
            std::vector<const double *> dev(mine.size(), nullptr);
            if (!default_backend().resident_onehot((uint32_t)a.DIM, (uint32_t)mine.size(), syms.data(), offs.data(), dev.data(), w)) error("the backend could not build the leaf graphs on the device");
            for (size_t s = 0; s < mine.size(); ++s) nodes[mine[s]].res.graph.setDevSites(dev[s]);
        }
    }
    // (the leaves of a group share the model's frequencies: all leaves of the pass, or a family's when -F estimates them per family)
    auto leaf_profiles = [&](const std::vector<int> &leaves) {
        // SequenceGraph(seq, csprofile, model_factory.getModel(branch_length)) for every leaf in one
        // createProfile batch (SequenceGraph.h:111-121, CSProfile.cpp:175-225).
        if (a.kind != ALPHA_AA) error("context-specific profiles need the AA alphabet");
        const uint32_t ns = (uint32_t)leaves.size();
        std::vector<uint32_t> offs(ns + 1, 0);
        std::vector<uint64_t> out_offs(ns + 1, 0);
        std::vector<double> tau(ns), p_uniform((size_t)ns * 20), pi(20, 0.0);
        std::vector<const sequence_t *> seqs(ns);
        for (uint32_t s = 0; s < ns; ++s) {
            seqs[s] = &sequence_of(leaves[s]);
            offs[s + 1] = offs[s] + (uint32_t)seqs[s]->size();
            out_offs[s + 1] = out_offs[s] + (uint64_t)20 * (seqs[s]->size() + 2);
        }
        std::vector<int8_t> syms(offs[ns]);
        parallel_for(ns, [&](size_t s) {   // (a model per leaf — its branch length —: P(t) from the eigen form, 20 us each)
            int8_t *o = syms.data() + offs[s];
            for (int8_t c : *seqs[s]) *o++ = a.isValid(c) ? (int8_t)a.value(c) : (int8_t)20;
            Model m = fenv[(size_t)nodes[leaves[s]].fam].model_factory->getModel(nodes[leaves[s]].tree->getBranchLength());
            tau[s] = m.divergence / 0.8;
            if (s == 0) pi = m.pi;   // (the same for every leaf)
            for (int i = 0; i < 20; ++i) {  // model.P * Constant(1/20)
                double acc = 0;
                for (int j = 0; j < 20; ++j) acc += m.P[i + 20 * j] * (1.0 / 20);
                p_uniform[(size_t)s * 20 + i] = acc;
            }
        });
        bool on_device = false;
        if (resident_pass) {   // the profile matrices stay where the leaf's subtree is aligned (as the one-hot leaves above)
            Backend &be = default_backend();
            on_device = true;
            for (int w = 0; w < be.workers() && on_device; ++w) {
                std::vector<uint32_t> mine;
                for (uint32_t s = 0; s < ns; ++s) if (owner[(size_t)leaves[s]] == w) mine.push_back(s);
                if (mine.empty()) continue;
                std::vector<int8_t> sy;
                std::vector<uint32_t> of(mine.size() + 1, 0);
                std::vector<double> ta(mine.size()), pu(mine.size() * 20);
                for (size_t k = 0; k < mine.size(); ++k) {
                    const uint32_t s = mine[k];
                    sy.insert(sy.end(), syms.begin() + offs[s], syms.begin() + offs[s + 1]);
                    of[k + 1] = (uint32_t)sy.size();
                    ta[k] = tau[s];
                    std::copy(p_uniform.begin() + (size_t)s * 20, p_uniform.begin() + (size_t)s * 20 + 20, pu.begin() + k * 20);
                }
                std::vector<const double *> dev(mine.size(), nullptr);
                on_device = be.csprofile_create_batch_res(*csprofile, (uint32_t)mine.size(), sy.data(), of.data(), ta.data(), pi.data(), pu.data(), dev.data(), w);
                if (!on_device) { if (w != 0) error("the backend could not build the leaf profiles on the device"); break; }
                for (size_t k = 0; k < mine.size(); ++k) {
                    Node &nd = nodes[leaves[mine[k]]];
                    nd.res.graph = Graph(20, (index_t)seqs[mine[k]]->size() + 2, Graph::NoSites());
                    nd.res.graph.setDevSites(dev[k]);
                    nd.res.is_csprofile = true;
                }
            }
            if (on_device) be.farm_leaf_workers = std::max(be.farm_leaf_workers, be.workers());
        }
        std::vector<double> out(on_device ? 0 : out_offs[ns]);
        if (!on_device) {
            // the leaves are independent (SequenceGraph.h:111-121): dealt to the device contexts by length
            Backend &be = default_backend();
            std::vector<uint64_t> cost(ns);
            for (uint32_t s = 0; s < ns; ++s) cost[s] = offs[s + 1] - offs[s];
            const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, be.workers());
            if (shards.size() <= 1) {
                be.csprofile_create_batch(*csprofile, ns, syms.data(), offs.data(), tau.data(), pi.data(), p_uniform.data(), out.data(), out_offs.data(), 0);
            } else {
                farm_run(shards, [&](int w) {
                    const std::vector<uint32_t> &sh = shards[(size_t)w];
                    const uint32_t m = (uint32_t)sh.size();
                    std::vector<int8_t> sy;
                    std::vector<uint32_t> of(m + 1, 0);
                    std::vector<uint64_t> oo(m + 1, 0);
                    std::vector<double> ta(m), pu((size_t)m * 20);
                    for (uint32_t k = 0; k < m; ++k) {
                        const uint32_t s = sh[k];
                        sy.insert(sy.end(), syms.begin() + offs[s], syms.begin() + offs[s + 1]);
                        of[k + 1] = (uint32_t)sy.size();
                        oo[k + 1] = oo[k] + (out_offs[s + 1] - out_offs[s]);
                        ta[k] = tau[s];
                        std::copy(p_uniform.begin() + (size_t)s * 20, p_uniform.begin() + (size_t)s * 20 + 20, pu.begin() + (size_t)k * 20);
                    }
                    std::vector<double> o(oo[m]);
                    be.csprofile_create_batch(*csprofile, m, sy.data(), of.data(), ta.data(), pi.data(), pu.data(), o.data(), oo.data(), w);
                    for (uint32_t k = 0; k < m; ++k) std::copy(o.begin() + oo[k], o.begin() + oo[k + 1], out.begin() + out_offs[sh[k]]);
                });
            }
            be.farm_leaf_workers = std::max(be.farm_leaf_workers, (int)shards.size());
        }
        for (uint32_t s = 0; s < ns && !on_device; ++s) {
            Node &nd = nodes[leaves[s]];
            index_t nn = (index_t)((out_offs[s + 1] - out_offs[s]) / 20);
            std::vector<double> sites(out.begin() + out_offs[s], out.begin() + out_offs[s + 1]);
            nd.res.graph = SequenceGraphFromProfile(20, nn, sites);
            nd.res.is_csprofile = true;
        }
    };
    if (csprofile) {
        if (forest && cmdlineopts.aafreqs_flag) {
            std::vector<std::vector<int>> of_family(families.size());
            for (int li : leaves) of_family[(size_t)nodes[(size_t)li].fam].push_back(li);
            for (const std::vector<int> &group : of_family) if (!group.empty()) leaf_profiles(group);
        } else leaf_profiles(leaves);
    }

    for (size_t f = 0; f < families.size(); ++f) {
        if (!fenv[f].with_repeats() || roots[f] < 0) continue;
        std::vector<int> mine;
        for (int li : leaves) if (nodes[(size_t)li].fam == (int)f) mine.push_back(li);
        attach_repeats(nodes, mine, fenv[f].repeats);
    }
    if (host_switches().profile)
        fprintf(stderr, "leaves: %zu, %.1f ms (names / owners %.2f, graphs %.2f, profiles %.2f)\n", leaves.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count(),
                std::chrono::duration<double, std::milli>(tl1 - tl0).count(), std::chrono::duration<double, std::milli>(tl2 - tl1).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl2).count());
    // ---- internal nodes, one guide-tree level per batch (ProgressiveAlignment.h:413-476) ----
    const LevelEnv env{a, fenv, resident_pass, cmdlineopts.earlyref_flag, false, tl0};
    for (int h = 1; h <= maxh; ++h) {
        std::vector<int> level;
        for (size_t i = 0; i < nodes.size(); ++i)
            if (nodes[i].height == h) level.push_back((int)i);
        run_level(env, nodes, owner, level, h);
        ++batch_stats.levels;
    }
    if (cmdlineopts.repeats_flag)   // the reference prints them as its recursion returns: post-order, which is the order of `nodes`
        for (const Node &nd : nodes) if (!nd.tr_note.empty()) std::cerr << nd.tr_note << std::endl;
    for (size_t f = 0; f < families.size(); ++f)
        if (roots[f] >= 0) *families[f].result = std::move(nodes[(size_t)roots[f]].res);
    if (host_switches().profile)
        fprintf(stderr, "[%.1f ms] root result taken\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count());
    nodes.clear();
    if (host_switches().profile)
        fprintf(stderr, "[%.1f ms] nodes released\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count());
}

// the forest of one tree
ProgressiveAlignmentResult progressive_alignment(const Alphabet &a, const std::map<std::string, sequence_t> &sequences,
                                                 const PhyTree &tree, const CSProfile *csprofile,
                                                 const ModelFactory &model_factory,
                                                 const std::map<std::string, std::vector<repeat_t>> *repeats) {
    ProgressiveAlignmentResult out;
    std::vector<ForestFamily> one(1);
    one[0].sequences = &sequences; one[0].tree = &tree; one[0].model_factory = &model_factory; one[0].repeats = repeats; one[0].result = &out;
    progressive_alignment_forest(a, one, csprofile);
    if (!one[0].error.empty()) throw pgm_exception(one[0].error);
    return out;
}

// ==== root search (FindRoot.h, GapParsimony.h) =====================================================================
// The reference memoises one alignment per directed subtree of the unrooted guide tree (node::getAlignment) and one per branch
// (edge::getAlignment), computing them on demand in its recursion.  Here they are the nodes of a DAG of merges, run height by
// height through run_level like the levels of a plain pass.  Rows are not carried through the DAG: every merge keeps its two
// mappings and a gap mask of its rows (one bit per column), which is all the gap parsimony reads; the winner's rows are
// composed from the mappings at the end.
RootSearchStats root_search_stats;

namespace {
struct UNode { int edges[3] = {-1, -1, -1}; const PhyTree *tree = nullptr; };   // edges[0]: toward the original root
struct UEdge { int nodes[2] = {-1, -1}; double length = -1, support = -1; };      // nodes[0]: the parent side
struct UGraph {
    std::vector<UNode> nodes;
    std::vector<UEdge> edges;
    bool isLeaf(int n) const { return nodes[(size_t)n].edges[1] < 0; }
    int other(int e, int n) const { return edges[(size_t)e].nodes[0] == n ? edges[(size_t)e].nodes[1] : edges[(size_t)e].nodes[0]; }
    int slot(int n, int e) const { for (int j = 0; j < 3; ++j) if (nodes[(size_t)n].edges[j] == e) return j; error("invalid edge"); }
};
struct GapMask {
    std::vector<uint64_t> bits;   // rows.size() x ceil(ncols / 64) words (include/pgm_hip.h)
    uint32_t ncols = 0;
    std::vector<int> rows;        // the graph leaves of the rows, in order
    int refs = 0;                 // merges that still extend it
};
}  // namespace

// tree2graph (FindRoot.h:176-234): edges in creation order, the edge to child 0 and its whole subtree before the edge to child 1
static void tree2graph(UGraph &g, int current, const PhyTree &tree) {
    g.nodes[(size_t)current].tree = &tree;
    if (tree.isLeaf()) return;
    if (tree.n_children() != 2) error("multifurcations not allowed");
    for (int i = 0; i < 2; ++i) {
        const int e = (int)g.edges.size(), n = (int)g.nodes.size();
        g.edges.push_back(UEdge());
        g.nodes.push_back(UNode());
        g.edges[(size_t)e].length = tree[i].getBranchLength();
        g.edges[(size_t)e].support = tree[i].getBranchSupport();
        g.edges[(size_t)e].nodes[0] = current; g.edges[(size_t)e].nodes[1] = n;
        g.nodes[(size_t)current].edges[1 + i] = e;
        g.nodes[(size_t)n].edges[0] = e;
        tree2graph(g, n, tree[i]);
    }
}

// FindRoot.h:242-275: a bifurcating root becomes one edge (lengths summed, the larger support), a trifurcating one a node of three
static UGraph unrooted_graph(const PhyTree &tree) {
    UGraph g;
    if (tree.n_children() == 2) {
        UEdge e0;
        e0.length = tree[0].getBranchLength() + tree[1].getBranchLength();
        e0.support = std::max(tree[0].getBranchSupport(), tree[1].getBranchSupport());
        e0.nodes[0] = 0; e0.nodes[1] = 1;
        g.edges.push_back(e0);
        g.nodes.resize(2);
        g.nodes[0].edges[0] = 0; g.nodes[1].edges[0] = 0;
        tree2graph(g, 0, tree[0]);
        tree2graph(g, 1, tree[1]);
    } else if (tree.n_children() == 3) {
        g.nodes.resize(1);
        for (int i = 0; i < 3; ++i) {
            const int e = (int)g.edges.size(), n = (int)g.nodes.size();
            g.edges.push_back(UEdge());
            g.nodes.push_back(UNode());
            g.edges[(size_t)e].length = tree[i].getBranchLength();
            g.edges[(size_t)e].support = tree[i].getBranchSupport();
            g.edges[(size_t)e].nodes[0] = 0; g.edges[(size_t)e].nodes[1] = n;
            g.nodes[(size_t)n].edges[0] = e;
            g.nodes[0].edges[i] = e;
            tree2graph(g, n, tree[i]);
        }
    } else {
        error("multifurcations not allowed");
    }
    return g;
}

// the host's own code behind Backend::gapmask_extend_batch / gap_parsimony_batch (same bits)
static void gapmask_extend_host(const pgm_gapmask_job &j) {
    const uint32_t wi = (j.ncols_in + 63) / 64, wo = (j.ncols_out + 63) / 64;
    uint32_t mapped = 0;
    for (uint32_t c = 0; c < j.ncols_out; ++c) mapped += j.mapping[c] != PGM_GAP;
    if (mapped != j.ncols_in) error("gap mask: the mapping does not cover the child's columns");
    for (uint32_t r = 0; r < j.nrows; ++r) {
        const uint64_t *src = j.src + (size_t)r * wi;
        uint64_t *dst = j.dst + (size_t)r * wo;
        std::fill(dst, dst + wo, 0ull);
        uint32_t k = 0;
        for (uint32_t c = 0; c < j.ncols_out; ++c) {
            uint64_t bit = 1;
            if (j.mapping[c] != PGM_GAP) { bit = (src[k >> 6] >> (k & 63)) & 1ull; ++k; }
            dst[c >> 6] |= bit << (c & 63);
        }
    }
}
static uint64_t spread32(uint32_t v) {   // bit c to bit 2c
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// GapParsimony.h:22-125 on a post-order topology: blocks of 32 columns, bit 2c residue, bit 2c + 1 gap; the padding loop's ones
// (the whole last block when the length is a multiple of 32)
static uint32_t gap_parsimony_host(const pgm_parsimony_job &j) {
    const uint32_t nb = (j.ncols + 31) / 32, words = (j.ncols + 63) / 64, ninner = j.nleaves - 1;
    std::vector<uint64_t> cons((size_t)ninner * nb);
    auto leaf = [&](uint32_t row, uint32_t b) {
        const uint32_t g = (uint32_t)(j.masks[(size_t)row * words + (b >> 1)] >> (32u * (b & 1u)));
        const uint32_t nv = b + 1 < nb ? 32u : j.ncols % 32u;
        const uint32_t vm = nv == 32u ? 0xFFFFFFFFu : (1u << nv) - 1u;
        return spread32(~g & vm) | (spread32(g & vm) << 1) | (spread32(~vm) * 3ull);
    };
    uint32_t score = 0;
    for (uint32_t k = 0; k < ninner; ++k)
        for (uint32_t b = 0; b < nb; ++b) {
            uint64_t w[2];
            for (int s = 0; s < 2; ++s) {
                const uint32_t c = j.children[2 * (size_t)k + s];
                w[s] = c < j.nleaves ? leaf(c, b) : cons[(size_t)(c - j.nleaves) * nb + b];
            }
            const uint64_t x = w[0] & w[1];
            uint64_t t = ~x;
            t = t & (t << 1) & 0xAAAAAAAAAAAAAAAAull;
            score += (uint32_t)__builtin_popcountll(t);
            cons[(size_t)k * nb + b] = x | t | (t >> 1);
        }
    return score;
}

namespace {
struct RootSearch {
    const Alphabet &a;
    const std::map<std::string, sequence_t> &sequences;
    const LevelEnv &env;
    UGraph g;
    std::vector<Node> nodes;                  // the DAG: leaves, directed results, candidates
    std::vector<GapMask> mask;
    std::vector<std::array<int, 3>> dres;     // graph node, edge slot -> DAG node of the node's result seen from that edge
    std::vector<int> cand;                    // edge -> DAG node of its candidate
    std::vector<double> score;                // edge -> gap parsimony score (-1: not yet)
    std::vector<char> done;
    std::vector<int> owner;
    // the batch bound: the cells of the largest alignGraphs batch the kernels have been tested with (the headline family's top levels)
    static constexpr double MAX_BATCH_CELLS = 2.7e8;

    RootSearch(const Alphabet &a_, const std::map<std::string, sequence_t> &seqs, const LevelEnv &e, const PhyTree &tree)
        : a(a_), sequences(seqs), env(e), g(unrooted_graph(tree)) {
        dres.assign(g.nodes.size(), std::array<int, 3>{{-1, -1, -1}});
        cand.assign(g.edges.size(), -1);
        score.assign(g.edges.size(), -1.0);
    }
    int add_node(Node &&n) {
        nodes.push_back(std::move(n));
        mask.push_back(GapMask());
        done.push_back(0);
        return (int)nodes.size() - 1;
    }
    // the consumers a directed result has in the full DAG: the results of the node across its edge seen from that node's other
    // edges, and the candidate of the edge itself
    int consumers(int n, int s) const {
        const int m = g.other(g.nodes[(size_t)n].edges[s], n);
        int deg = 0;
        for (int j = 0; j < 3; ++j) deg += g.nodes[(size_t)m].edges[j] >= 0;
        return deg;
    }
    // node::getAlignment (FindRoot.h:85-122): the results of the two other neighbours, ascending edge slots
    int directed(int n, int s) {
        if (dres[(size_t)n][(size_t)s] >= 0) return dres[(size_t)n][(size_t)s];
        Node nd;
        nd.tree = nullptr;
        if (g.isLeaf(n)) {
            nd.tree = g.nodes[(size_t)n].tree;
        } else {
            const int i1 = s == 0 ? 1 : 0, i2 = s == 2 ? 1 : 2;
            const int sl[2] = {i1, i2};
            for (int c = 0; c < 2; ++c) {
                const int e = g.nodes[(size_t)n].edges[sl[c]], m = g.other(e, n);
                nd.child[c] = directed(m, g.slot(m, e));
                nd.len[c] = g.edges[(size_t)e].length;
                nd.sup[c] = g.edges[(size_t)e].support;
            }
            nd.height = 1 + std::max(nodes[(size_t)nd.child[0]].height, nodes[(size_t)nd.child[1]].height);
        }
        nd.refs = consumers(n, s);
        const int id = add_node(std::move(nd));
        mask[(size_t)id].refs = nodes[(size_t)id].refs;
        if (g.isLeaf(n)) mask[(size_t)id].rows.assign(1, n);
        dres[(size_t)n][(size_t)s] = id;
        return id;
    }
    // edge::getAlignment (FindRoot.h:124-134): the two sides at half the edge's length each, its support on both
    int candidate(int e) {
        if (cand[(size_t)e] >= 0) return cand[(size_t)e];
        const UEdge &ue = g.edges[(size_t)e];
        Node nd;
        nd.tree = nullptr;
        for (int c = 0; c < 2; ++c) {
            const int m = ue.nodes[c];
            nd.child[c] = directed(m, g.slot(m, e));
            nd.len[c] = ue.length / 2;
            nd.sup[c] = ue.support;
        }
        nd.height = 1 + std::max(nodes[(size_t)nd.child[0]].height, nodes[(size_t)nd.child[1]].height);
        const int id = add_node(std::move(nd));
        cand[(size_t)e] = id;
        return id;
    }

    void build_leaves(const std::vector<int> &leaves) {
        const bool resident_leaves = env.resident_pass;
        parallel_for(leaves.size(), [&](size_t k) {
            Node &nd = nodes[(size_t)leaves[k]];
            const sequence_t &seq = sequences.at(nd.tree->getName());
            nd.res.score = 0;
            nd.res.n_tr_indels = 0;
            nd.res.is_csprofile = false;   // (the header's tree2graph: plain sequence graphs even with -c, FindRoot.h:183)
            nd.res.graph = resident_leaves ? Graph(a.DIM, (index_t)seq.size() + 2, Graph::NoSites()) : SequenceGraph(a, seq);
            GapMask &m = mask[(size_t)leaves[k]];
            m.ncols = (uint32_t)seq.size();
            m.bits.assign((seq.size() + 63) / 64, 0ull);
            for (size_t c = 0; c < seq.size(); ++c) if (a.isGap(seq[c])) m.bits[c >> 6] |= 1ull << (c & 63);
            done[(size_t)leaves[k]] = 1;
        });
        if (resident_leaves && !leaves.empty()) {
            std::vector<uint32_t> offs(leaves.size() + 1, 0);
            for (size_t s = 0; s < leaves.size(); ++s) offs[s + 1] = offs[s] + (uint32_t)sequences.at(nodes[(size_t)leaves[s]].tree->getName()).size();
            std::vector<int8_t> syms(offs[leaves.size()]);
            parallel_for(leaves.size(), [&](size_t s) {
                int8_t *out = syms.data() + offs[s];
                for (int8_t c : sequences.at(nodes[(size_t)leaves[s]].tree->getName())) *out++ = a.isValid(c) ? (int8_t)a.value(c) : (int8_t)-1;
            });
            std::vector<const double *> dev(leaves.size(), nullptr);
            if (!default_backend().resident_onehot((uint32_t)a.DIM, (uint32_t)leaves.size(), syms.data(), offs.data(), dev.data(), 0)) error("the backend could not build the leaf graphs on the device");
            for (size_t s = 0; s < leaves.size(); ++s) nodes[(size_t)leaves[s]].res.graph.setDevSites(dev[s]);
        }
        attach_repeats(nodes, leaves, env.fams[0].repeats);
    }

    // the gap masks of a height's merges: each child's rows through the merge's mapping, in one backend call
    void extend_masks(const std::vector<int> &level) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<pgm_gapmask_job> jobs;
        for (int v : level) {
            Node &nd = nodes[(size_t)v];
            GapMask &m = mask[(size_t)v];
            const size_t n = nd.map[0].size();
            if (n < 2 || nd.map[1].size() != n) error("root search: inconsistent merge mappings");
            m.ncols = (uint32_t)(n - 2);
            const size_t words = (m.ncols + 63) / 64;
            const GapMask &m0 = mask[(size_t)nd.child[0]], &m1 = mask[(size_t)nd.child[1]];
            m.rows = m0.rows;
            m.rows.insert(m.rows.end(), m1.rows.begin(), m1.rows.end());
            m.bits.assign(m.rows.size() * words, 0ull);
            size_t row = 0;
            for (int c = 0; c < 2; ++c) {
                const GapMask &cm = mask[(size_t)nd.child[c]];
                pgm_gapmask_job j;
                j.src = cm.bits.data(); j.mapping = nd.map[c].data() + 1; j.dst = m.bits.data() + row * words;
                j.nrows = (uint32_t)cm.rows.size(); j.ncols_in = cm.ncols; j.ncols_out = m.ncols;
                jobs.push_back(j);
                row += cm.rows.size();
            }
        }
        if (!jobs.empty() && !default_backend().gapmask_extend_batch((uint32_t)jobs.size(), jobs.data(), 0))
            parallel_for(jobs.size(), [&](size_t q) { gapmask_extend_host(jobs[q]); });
        for (int v : level)
            for (int c = 0; c < 2; ++c) {
                GapMask &cm = mask[(size_t)nodes[(size_t)v].child[c]];
                if (--cm.refs == 0) cm = GapMask();
            }
        root_search_stats.gapmask_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }

    // the rooted topology of the candidate of edge e over the rows of its mask: post-order, the root last
    uint32_t topo(int n, int from, const std::vector<int> &row_of, std::vector<uint32_t> &children, uint32_t nleaves) const {
        if (g.isLeaf(n)) return (uint32_t)row_of[(size_t)n];
        uint32_t c[2];
        int k = 0;
        for (int j = 0; j < 3; ++j) {
            const int e = g.nodes[(size_t)n].edges[j];
            if (e == from || e < 0) continue;
            c[k++] = topo(g.other(e, n), e, row_of, children, nleaves);
        }
        children.push_back(c[0]); children.push_back(c[1]);
        return nleaves + (uint32_t)(children.size() / 2 - 1);
    }
    void score_candidates(const std::vector<int> &edges) {
        if (edges.empty()) return;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<uint32_t>> children(edges.size());
        std::vector<pgm_parsimony_job> jobs(edges.size());
        std::vector<int> row_of(g.nodes.size(), -1);
        for (size_t q = 0; q < edges.size(); ++q) {
            const int e = edges[q];
            const GapMask &m = mask[(size_t)cand[(size_t)e]];
            for (size_t r = 0; r < m.rows.size(); ++r) row_of[(size_t)m.rows[r]] = (int)r;
            const uint32_t nl = (uint32_t)m.rows.size();
            const uint32_t c0 = topo(g.edges[(size_t)e].nodes[0], e, row_of, children[q], nl);
            const uint32_t c1 = topo(g.edges[(size_t)e].nodes[1], e, row_of, children[q], nl);
            children[q].push_back(c0); children[q].push_back(c1);
            jobs[q].masks = m.bits.data(); jobs[q].children = children[q].data(); jobs[q].nleaves = nl; jobs[q].ncols = m.ncols;
            if (nl < 2 || m.ncols == 0) error("root search: a candidate alignment without rows or columns");
        }
        std::vector<uint32_t> sc(edges.size(), 0);
        if (!default_backend().gap_parsimony_batch((uint32_t)jobs.size(), jobs.data(), sc.data(), 0))
            parallel_for(jobs.size(), [&](size_t q) { sc[q] = gap_parsimony_host(jobs[q]); });
        for (size_t q = 0; q < edges.size(); ++q) {
            score[(size_t)edges[q]] = (score_t)sc[q];   // (unsigned -> score_t, FindRoot.h:279)
            const int c = cand[(size_t)edges[q]];
            mask[(size_t)c] = GapMask();
            nodes[(size_t)c].res.graph = Graph();   // (score and TR indels stay; the rows are composed from the mappings)
            nodes[(size_t)c].res.tr_homologies.clear();
            nodes[(size_t)c].res.tr_source.clear();
        }
        root_search_stats.parsimony_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }

    // every merge the candidates of `edges` still need, height by height; then their scores
    void evaluate(const std::vector<int> &edges) {
        std::vector<int> todo;
        for (int e : edges) if (score[(size_t)e] < 0) todo.push_back(e);
        if (todo.empty()) return;
        for (int e : todo) candidate(e);
        std::vector<std::vector<int>> by_height;
        std::vector<char> seen(nodes.size(), 0);
        std::vector<int> stack;
        for (int e : todo) stack.push_back(cand[(size_t)e]);
        while (!stack.empty()) {
            const int v = stack.back(); stack.pop_back();
            if (seen[(size_t)v] || done[(size_t)v]) continue;
            seen[(size_t)v] = 1;
            const Node &nd = nodes[(size_t)v];
            if ((size_t)nd.height >= by_height.size()) by_height.resize((size_t)nd.height + 1);
            by_height[(size_t)nd.height].push_back(v);
            if (nd.child[0] >= 0) { stack.push_back(nd.child[0]); stack.push_back(nd.child[1]); }
        }
        owner.assign(nodes.size(), 0);
        if (!by_height.empty() && !by_height[0].empty()) build_leaves(by_height[0]);
        for (size_t h = 1; h < by_height.size(); ++h) {
            std::vector<int> &level = by_height[h];
            if (level.empty()) continue;
            std::sort(level.begin(), level.end());
            // a height above the batch bound goes in several batches
            std::vector<int> chunk;
            double cells = 0;
            const auto t0 = std::chrono::steady_clock::now();
            const double align0 = default_backend().seconds_align;
            auto flush = [&]() {
                if (chunk.empty()) return;
                run_level(env, nodes, owner, chunk, (int)h);
                ++root_search_stats.batches;
                chunk.clear();
                cells = 0;
            };
            for (int v : level) {
                const Node &nd = nodes[(size_t)v];
                const double c = (double)(nodes[(size_t)nd.child[0]].res.graph.size() - 2) * (double)(nodes[(size_t)nd.child[1]].res.graph.size() - 2);
                if (!chunk.empty() && cells + c > MAX_BATCH_CELLS) flush();
                chunk.push_back(v);
                cells += c;
            }
            flush();
            const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), align = default_backend().seconds_align - align0;
            root_search_stats.align_s += align;
            root_search_stats.host_merge_s += wall - align;
            root_search_stats.merges += (int)level.size();
            ++root_search_stats.heights;
            for (int v : level) done[(size_t)v] = 1;
            extend_masks(level);
            std::vector<int> scored;
            for (int e : todo) if (cand[(size_t)e] >= 0 && nodes[(size_t)cand[(size_t)e]].height == (int)h) scored.push_back(e);
            score_candidates(scored);
            root_search_stats.candidates += (int)scored.size();
        }
    }

    // the winner's rows: extend_alignment down its sub-DAG, composed from the kept mappings
    std::map<std::string, sequence_t> rows(int v) const {
        const Node &nd = nodes[(size_t)v];
        std::map<std::string, sequence_t> out;
        if (nd.child[0] < 0) {
            out[nd.tree->getName()] = sequences.at(nd.tree->getName());
            return out;
        }
        for (int c = 0; c < 2; ++c) {
            const std::map<std::string, sequence_t> r = rows(nd.child[c]);
            extend_rows(a, out, (index_t)nd.map[c].size(), nd.map[c], r, r.size() >= 64);
        }
        return out;
    }
};
}  // namespace

ProgressiveAlignmentResult progressive_alignment_find_root(const Alphabet &a, const std::map<std::string, sequence_t> &sequences,
                                                           const PhyTree &tree, const ModelFactory &model_factory,
                                                           const std::map<std::string, std::vector<repeat_t>> *repeats) {
    if (!cmdlineopts.profile_file.empty() || cmdlineopts.ancestral_flag) error("--profile_out and --ancestral_seqs cannot be combined with -r");
    const auto t0 = std::chrono::steady_clock::now();
    Backend &be = default_backend();
    be.resident_reset();
    // one device context (worker 0); the root search keeps no early refinement (FindRoot.h calls align_progressive_results only)
    const bool resident_pass = be.resident() && !host_switches().host_merge && !job_dump_active();
    be.resident_pass = resident_pass;
    be.resident_imports = 0;
    root_search_stats = RootSearchStats();
    root_search_stats.ran = true;
    const LevelEnv env{a, {FamEnv{&model_factory, repeats}}, resident_pass, false, true, t0};
    RootSearch rs(a, sequences, env, tree);
    for (size_t n = 0; n < rs.g.nodes.size(); ++n)
        if (rs.g.isLeaf((int)n) && !sequences.count(rs.g.nodes[n].tree->getName())) error("unknown sequence name: %s", rs.g.nodes[n].tree->getName().c_str());
    const int E = (int)rs.g.edges.size();
    int best_edge = 0;
    if (cmdlineopts.reroot_flag == 1) {   // every branch, the first minimum in edge order (FindRoot.h:281-289)
        std::vector<int> all(E);
        for (int e = 0; e < E; ++e) all[(size_t)e] = e;
        rs.evaluate(all);
        for (int e = 1; e < E; ++e) if (rs.score[(size_t)e] < rs.score[(size_t)best_edge]) best_edge = e;
    } else {   // hill climbing over the neighbouring branches (FindRoot.h:290-320), one iteration's candidates per batch
        rs.evaluate({0});
        int best_node = -1;
        score_t best_score = rs.score[0];
        for (;;) {
            const int old_edge = best_edge, old_node = best_node;
            std::vector<std::pair<int, int>> tries;
            for (int i = 0; i < 2; ++i) {
                const int n = rs.g.edges[(size_t)old_edge].nodes[i];
                if (n == old_node) continue;
                for (int j = 0; j < 3; ++j) {
                    const int e = rs.g.nodes[(size_t)n].edges[j];
                    if (e == old_edge || e < 0) continue;
                    tries.emplace_back(n, e);
                }
            }
            std::vector<int> es;
            for (const auto &t : tries) es.push_back(t.second);
            rs.evaluate(es);
            for (const auto &t : tries)
                if (rs.score[(size_t)t.second] < best_score) { best_edge = t.second; best_score = rs.score[(size_t)t.second]; best_node = t.first; }
            if (best_edge == old_edge) break;
        }
    }
    const score_t best_score = rs.score[(size_t)best_edge];
    std::cerr << "best gap parsimony score: " << best_score << std::endl;
    const auto ts = std::chrono::steady_clock::now();
    const int w = rs.cand[(size_t)best_edge];
    ProgressiveAlignmentResult result;
    result.score = rs.nodes[(size_t)w].res.score;
    result.n_tr_indels = rs.nodes[(size_t)w].res.n_tr_indels;
    result.aligned_sequences = rs.rows(w);
    root_search_stats.select_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
    if (host_switches().profile)
        fprintf(stderr, "root search: %d merges in %d heights (%d batches), %d candidates; align %.1f ms, host merges %.1f, gap masks %.1f, parsimony %.1f, rows %.1f\n",
                root_search_stats.merges, root_search_stats.heights, root_search_stats.batches, root_search_stats.candidates, root_search_stats.align_s * 1e3,
                root_search_stats.host_merge_s * 1e3, root_search_stats.gapmask_s * 1e3, root_search_stats.parsimony_s * 1e3, root_search_stats.select_s * 1e3);
    return result;
}

// ==== --guidance: residue map, agreement counts on the host, score files ===============================================
#include "guidance.inc"

// ==== --bootstrap_tbe: transfer indices on the host, the support of every edge ========================================
#include "transfer.inc"

}  // namespace pgm
