// progressive.cpp — progressive alignment driver (reference src/ProgressiveAlignment.{h,cpp}).
//
// The reference recurses strictly sequentially (ProgressiveAlignment.cpp:50-51).  The results of
// sibling subtrees are independent, so this driver walks the tree level by level ("height" = longest
// path to a leaf) and hands every ready internal node of a level to the backend in ONE batched
// alignGraphs call; the per-node host work (CleanedGraph, mergeGraphs, extend_alignment) runs on a
// few host threads.  The values produced per node are those of the reference's recursion.
// Here: the pass over a forest of guide trees (the leaf stage, then run_level per height), early refinement and ancestral
// sequences.  The root search (root_search.cpp) runs its DAG of merges through the same run_level.
#include "progressive_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <iostream>
#include <thread>

namespace pgm {

void extend_rows(const Alphabet &a, std::map<std::string, sequence_t> &out, index_t n, const std::vector<index_t> &mapping,
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
            extend_rows(a, result.aligned_sequences, result.graph.size(), mappings[i], dr.aligned_sequences, false);
            extend_tr_homologies(result, mappings[i], dr.tr_homologies, dr.tr_source);
        }
        if (fams[(size_t)nd.fam].with_repeats()) result.graph.addRepeats(result.tr_homologies);
        nd.res = std::move(result);
    });
}

// ---- the leaf stage (ProgressiveAlignment.cpp:17-46) ----
void init_leaf(const Alphabet &a, ProgressiveAlignmentResult &res, const sequence_t &seq, LeafGraph graph, const std::string *row_name) {
    if (row_name) res.aligned_sequences[*row_name] = seq;
    res.score = 0;
    res.n_tr_indels = 0;
    res.is_csprofile = false;
    if (graph == LeafGraph::OnDevice) res.graph = Graph(a.DIM, (index_t)seq.size() + 2, Graph::NoSites());
    else if (graph == LeafGraph::OnHost) res.graph = SequenceGraph(a, seq);
}

void upload_onehot_leaves(const Alphabet &a, std::vector<Node> &nodes, const std::vector<int> &leaves, const std::vector<const sequence_t *> &seq_of, int worker) {
    if (leaves.empty()) return;
    std::vector<uint32_t> offs(leaves.size() + 1, 0);
    for (size_t s = 0; s < leaves.size(); ++s) offs[s + 1] = offs[s] + (uint32_t)seq_of[(size_t)leaves[s]]->size();
    std::vector<int8_t> syms(offs[leaves.size()]);
    parallel_for(leaves.size(), [&](size_t s) {   // (a quarter of a million residues one push_back at a time: 1 ms of the leaf stage)
        int8_t *out = syms.data() + offs[s];
        for (int8_t c : *seq_of[(size_t)leaves[s]]) *out++ = a.isValid(c) ? (int8_t)a.value(c) : (int8_t)-1;
    });
    std::vector<const double *> dev(leaves.size(), nullptr);
    if (!default_backend().resident_onehot((uint32_t)a.DIM, (uint32_t)leaves.size(), syms.data(), offs.data(), dev.data(), worker)) error("the backend could not build the leaf graphs on the device");
    for (size_t s = 0; s < leaves.size(); ++s) nodes[(size_t)leaves[s]].res.graph.setDevSites(dev[s]);
}

namespace {
// the arguments of one createProfile batch, per leaf: the symbols (20: not valid) between offs, tau and model.P * Constant(1/20) of
// the leaf's model, and where its 20 x (len + 2) matrix goes in the output of the host path
struct CsLeafBatch {
    std::vector<int8_t> syms;
    std::vector<uint32_t> offs;
    std::vector<uint64_t> out_offs;
    std::vector<double> tau, p_uniform;
    explicit CsLeafBatch(size_t m) : offs(m + 1, 0), out_offs(m + 1, 0), tau(m), p_uniform(m * 20) {}
    CsLeafBatch subset(const std::vector<uint32_t> &pick) const {
        CsLeafBatch q(pick.size());
        for (size_t k = 0; k < pick.size(); ++k) {
            const uint32_t s = pick[k];
            q.syms.insert(q.syms.end(), syms.begin() + offs[s], syms.begin() + offs[s + 1]);
            q.offs[k + 1] = (uint32_t)q.syms.size();
            q.out_offs[k + 1] = q.out_offs[k] + (out_offs[s + 1] - out_offs[s]);
            q.tau[k] = tau[s];
            std::copy(p_uniform.begin() + (size_t)s * 20, p_uniform.begin() + (size_t)s * 20 + 20, q.p_uniform.begin() + k * 20);
        }
        return q;
    }
};
}  // namespace

// SequenceGraph(seq, csprofile, model_factory.getModel(branch_length)) for every leaf of `leaves` (seq_of: by node) in one
// createProfile batch (SequenceGraph.h:111-121, CSProfile.cpp:175-225).  The leaves of a call share the model's frequencies: all
// leaves of the pass, or a family's when -F estimates them per family.
static void csprofile_leaves(const Alphabet &a, const CSProfile &csprofile, const std::vector<FamEnv> &fenv, std::vector<Node> &nodes, const std::vector<int> &leaves,
                             const std::vector<const sequence_t *> &seq_of, bool resident_pass, const std::vector<int> &owner) {
    if (a.kind != ALPHA_AA) error("context-specific profiles need the AA alphabet");
    const uint32_t ns = (uint32_t)leaves.size();
    CsLeafBatch all(ns);
    std::vector<double> pi(20, 0.0);
    for (uint32_t s = 0; s < ns; ++s) {
        const size_t len = seq_of[(size_t)leaves[s]]->size();
        all.offs[s + 1] = all.offs[s] + (uint32_t)len;
        all.out_offs[s + 1] = all.out_offs[s] + (uint64_t)20 * (len + 2);
    }
    all.syms.resize(all.offs[ns]);
    parallel_for(ns, [&](size_t s) {   // (a model per leaf — its branch length —: P(t) from the eigen form, 20 us each)
        int8_t *o = all.syms.data() + all.offs[s];
        for (int8_t c : *seq_of[(size_t)leaves[s]]) *o++ = a.isValid(c) ? (int8_t)a.value(c) : (int8_t)20;
        Model m = fenv[(size_t)nodes[(size_t)leaves[s]].fam].model_factory->getModel(nodes[(size_t)leaves[s]].tree->getBranchLength());
        all.tau[s] = m.divergence / 0.8;
        if (s == 0) pi = m.pi;   // (the same for every leaf)
        for (int i = 0; i < 20; ++i) {  // model.P * Constant(1/20)
            double acc = 0;
            for (int j = 0; j < 20; ++j) acc += m.P[i + 20 * j] * (1.0 / 20);
            all.p_uniform[s * 20 + i] = acc;
        }
    });
    Backend &be = default_backend();
    if (resident_pass) {   // the profile matrices stay where the leaf's subtree is aligned (as the one-hot leaves)
        bool on_device = true;
        for (int w = 0; w < be.workers() && on_device; ++w) {
            std::vector<uint32_t> mine;
            for (uint32_t s = 0; s < ns; ++s) if (owner[(size_t)leaves[s]] == w) mine.push_back(s);
            if (mine.empty()) continue;
            const CsLeafBatch q = all.subset(mine);
            std::vector<const double *> dev(mine.size(), nullptr);
            on_device = be.csprofile_create_batch_res(csprofile, (uint32_t)mine.size(), q.syms.data(), q.offs.data(), q.tau.data(), pi.data(), q.p_uniform.data(), dev.data(), w);
            if (!on_device) { if (w != 0) error("the backend could not build the leaf profiles on the device"); break; }
            for (size_t k = 0; k < mine.size(); ++k) {
                Node &nd = nodes[(size_t)leaves[mine[k]]];
                nd.res.graph = Graph(20, (index_t)(q.offs[k + 1] - q.offs[k]) + 2, Graph::NoSites());
                nd.res.graph.setDevSites(dev[k]);
                nd.res.is_csprofile = true;
            }
        }
        if (on_device) { be.farm_leaf_workers = std::max(be.farm_leaf_workers, be.workers()); return; }
    }
    // the host's profiles.  The leaves are independent (SequenceGraph.h:111-121): dealt to the device contexts by length
    std::vector<double> out(all.out_offs[ns]);
    std::vector<uint64_t> cost(ns);
    for (uint32_t s = 0; s < ns; ++s) cost[s] = all.offs[s + 1] - all.offs[s];
    const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, be.workers());
    if (shards.size() <= 1) {
        be.csprofile_create_batch(csprofile, ns, all.syms.data(), all.offs.data(), all.tau.data(), pi.data(), all.p_uniform.data(), out.data(), all.out_offs.data(), 0);
    } else {
        farm_run(shards, [&](int w) {
            const std::vector<uint32_t> &sh = shards[(size_t)w];
            const CsLeafBatch q = all.subset(sh);
            std::vector<double> o(q.out_offs[sh.size()]);
            be.csprofile_create_batch(csprofile, (uint32_t)sh.size(), q.syms.data(), q.offs.data(), q.tau.data(), pi.data(), q.p_uniform.data(), o.data(), q.out_offs.data(), w);
            for (size_t k = 0; k < sh.size(); ++k) std::copy(o.begin() + q.out_offs[k], o.begin() + q.out_offs[k + 1], out.begin() + all.out_offs[sh[k]]);
        });
    }
    be.farm_leaf_workers = std::max(be.farm_leaf_workers, (int)shards.size());
    for (uint32_t s = 0; s < ns; ++s) {
        Node &nd = nodes[(size_t)leaves[s]];
        index_t nn = (index_t)((all.out_offs[s + 1] - all.out_offs[s]) / 20);
        std::vector<double> sites(out.begin() + all.out_offs[s], out.begin() + all.out_offs[s + 1]);
        nd.res.graph = SequenceGraphFromProfile(20, nn, sites);
        nd.res.is_csprofile = true;
    }
}

// ---- a level of merges: align_progressive_results (ProgressiveAlignment.h:413-476) of every node of `level` in one batch ----
namespace {
struct Pending {  // state of one align_progressive_results call between its two halves
    Model model, model1, model2;
    std::unique_ptr<CleanedGraph> cg1, cg2;
};
// the state of one run_level call; everything is indexed by the position in `level`
struct LevelState {
    std::vector<Pending> pend;
    std::vector<int> worker_of;                  // the device context the node's job and merge run on: its owner
    std::vector<AlignmentResult> ar;
    std::vector<MergePlan> plans;
    std::vector<std::vector<double>> profiles;   // the merged graphs' node profiles on the host (not a resident pass)
    std::vector<const double *> dev_profiles;    // ... on the device (a resident pass)
    std::vector<pgm_merge_job> mj;
    std::chrono::steady_clock::time_point tp0, tp1, tp2, tq0, tq1;
    std::atomic<long long> ns_merge{0}, ns_extend{0};
    explicit LevelState(size_t L) : pend(L), worker_of(L, 0), plans(L), profiles(L), dev_profiles(L, nullptr), mj(L) {}
};
}  // namespace

// children of a node above the cut of the subtrees (a resident pass): the profiles of the one on another worker are copied over
static void import_children(const Alphabet &a, std::vector<Node> &nodes, std::vector<int> &owner, const std::vector<int> &level) {
    for (size_t k = 0; k < level.size(); ++k) {
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
}

// the models of every node's merge and the cleaned graphs of its children
static void prepare_level(const LevelEnv &env, const std::vector<Node> &nodes, const std::vector<int> &level, std::vector<Pending> &pend) {
    parallel_for(level.size(), [&](size_t k) {
        const Node &nd = nodes[level[k]];
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
}

// the level's alignGraphs batch (worker_of given: every job on the worker that holds its children's profiles)
static std::vector<AlignmentResult> align_level(const std::vector<Pending> &pend, const std::vector<int> *worker_of) {
    const size_t L = pend.size();
    std::vector<const Graph *> g1(L), g2(L);
    std::vector<const Model *> mm(L);
    for (size_t k = 0; k < L; ++k) { g1[k] = pend[k].cg1.get(); g2[k] = pend[k].cg2.get(); mm[k] = &pend[k].model; }
    // graphs merged on the device one level below: their profiles never left it (gathered there through the cleaned graphs' node maps)
    std::vector<pgm_site_ref> rs1, rs2;
    bool any = false;
    for (size_t k = 0; k < L; ++k) any = any || pend[k].cg1->devSites() || pend[k].cg2->devSites();
    if (any) {
        rs1.assign(L, pgm_site_ref{nullptr, nullptr, 0u}); rs2.assign(L, pgm_site_ref{nullptr, nullptr, 0u});
        for (size_t k = 0; k < L; ++k) {
            if (pend[k].cg1->devSites()) rs1[k] = pgm_site_ref{pend[k].cg1->devSites(), pend[k].cg1->nodeMap(), (uint32_t)pend[k].cg1->originalSize()};
            if (pend[k].cg2->devSites()) rs2[k] = pgm_site_ref{pend[k].cg2->devSites(), pend[k].cg2->nodeMap(), (uint32_t)pend[k].cg2->originalSize()};
        }
    }
    return alignGraphsBatch(g1, g2, mm, rs1, rs2, worker_of);
}

// mergeGraphs, first part: the plans of the level's merges on the host threads
static void plan_merges(const LevelEnv &env, const std::vector<Node> &nodes, const std::vector<int> &level, LevelState &st) {
    parallel_for(level.size(), [&](size_t k) {
        const Node &nd = nodes[level[k]];
        Pending &p = st.pend[k];
        p.cg1->uncleanMapping(st.ar[k].mapping1);
        p.cg2->uncleanMapping(st.ar[k].mapping2);
        st.plans[k] = planMerge(nodes[nd.child[0]].res.graph, nodes[nd.child[1]].res.graph, st.ar[k].mapping1, st.ar[k].mapping2);
        if (!env.resident_pass) st.profiles[k].assign((size_t)env.a.DIM * st.plans[k].mapping1.size(), 0.0);
    });
}

// The node profiles (P g products, L2 normalisation: the arithmetic of the merge) of the level's merges in one device batch per
// worker.  A resident pass: every merge where its children are, the profiles stay there, and the backend must not refuse.
// Otherwise the merges are independent: dealt to the device contexts by the size of the merged graph; false: a context refused,
// the host computes them (mergeProfilesHost).  One shard is the batch as it is.
static bool merge_profiles_on_device(LevelState &st, bool resident) {
    Backend &be = default_backend();
    const size_t L = st.mj.size();
    std::vector<std::vector<uint32_t>> shards;
    if (resident) {
        shards.resize((size_t)be.workers());
        for (size_t k = 0; k < L; ++k) shards[(size_t)st.worker_of[k]].push_back((uint32_t)k);
    } else {
        std::vector<uint64_t> cost(L);
        for (size_t k = 0; k < L; ++k) cost[k] = st.mj[k].nnodes;
        shards = farm_shards(cost, be.workers());
    }
    const bool whole = shards.size() == 1;
    std::vector<char> ok(shards.size(), 1);
    farm_run(shards, [&](int w) {
        const std::vector<uint32_t> &sh = shards[(size_t)w];
        const std::vector<pgm_merge_job> q = whole ? std::vector<pgm_merge_job>() : shard_pick(st.mj, sh);
        const pgm_merge_job *jobs = whole ? st.mj.data() : q.data();
        if (resident) {
            std::vector<const double *> dv(whole ? 0 : sh.size(), nullptr);
            ok[(size_t)w] = be.merge_profiles_batch_res((uint32_t)sh.size(), jobs, whole ? st.dev_profiles.data() : dv.data(), w) ? 1 : 0;
            for (size_t k = 0; k < dv.size(); ++k) st.dev_profiles[sh[k]] = dv[k];
        } else ok[(size_t)w] = be.merge_profiles_batch((uint32_t)sh.size(), jobs, w) ? 1 : 0;
    });
    bool on_device = true;
    for (char c : ok) on_device = on_device && c;
    if (resident && !on_device) error("the backend could not keep the merged profiles on the device");
    return on_device;
}

// mergeGraphs, last part, and the rest of align_progressive_results for every node on the host threads: the graph, the rows (the
// root search: the mappings), repeats, ancestral sequences; then the node's children and its scratch are let go.
// merge_on_host: the node profiles were not computed on the device
static void finish_nodes(const LevelEnv &env, std::vector<Node> &nodes, const std::vector<int> &level, LevelState &st, bool merge_on_host) {
    const Alphabet &a = env.a;
    const size_t L = level.size();
    parallel_for(L, [&](size_t k) {
        const auto tk0 = std::chrono::steady_clock::now();
        Node &nd = nodes[level[k]];
        ProgressiveAlignmentResult &r1 = nodes[nd.child[0]].res, &r2 = nodes[nd.child[1]].res;
        Pending &p = st.pend[k];
        const AlignmentResult &ar = st.ar[k];
        ProgressiveAlignmentResult &result = nd.res;
        result.score = ar.score;
        result.is_csprofile = false;
        result.n_tr_indels = ar.n_tr_indels + r1.n_tr_indels + r2.n_tr_indels;
        if (merge_on_host) mergeProfilesHost(r1.graph, r2.graph, p.model1, p.model2, st.plans[k], st.profiles[k]);
        AncestralResult anc = finishMerge(r1.graph, r2.graph, st.plans[k], env.resident_pass ? nullptr : st.profiles[k].data(), nd.sup[0], nd.sup[1]);
        result.graph = anc.graph;
        const auto tk1 = std::chrono::steady_clock::now();
        if (!env.dag) {
            extend_rows(a, result.aligned_sequences, result.graph.size(), anc.mapping1, r1.aligned_sequences, L == 1);
            extend_rows(a, result.aligned_sequences, result.graph.size(), anc.mapping2, r2.aligned_sequences, L == 1);
        } else {
            nd.map[0] = anc.mapping1;
            nd.map[1] = anc.mapping2;
        }
        st.ns_merge += std::chrono::duration_cast<std::chrono::nanoseconds>(tk1 - tk0).count();
        st.ns_extend += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tk1).count();
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
        if (cmdlineopts.repeats_flag && !env.dag) nd.tr_note = "TR indels at " + create_ancestral_seq_name(result.aligned_sequences) + ": " + std::to_string(ar.n_tr_indels);   // (:470-473)
        if (env.fams[(size_t)nd.fam].with_repeats()) result.graph.addRepeats(result.tr_homologies);   // (:468; with no annotation at all the merged graph has no repeat edges either way)
        // children are no longer needed (the reference copies them by value and drops them)
        if (!env.earlyref && !env.dag) {   // (the reference's alignment_cache, ProgressiveAlignment.h:107-109: the parent's refinement reads them again)
            r1 = ProgressiveAlignmentResult();
            r2 = ProgressiveAlignmentResult();
        }
        p.cg1.reset();
        p.cg2.reset();
        st.profiles[k] = std::vector<double>();
    });
}

void run_level(const LevelEnv &env, std::vector<Node> &nodes, std::vector<int> &owner, const std::vector<int> &level, int h) {
    const Alphabet &a = env.a;
    const size_t L = level.size();
    // The merged profiles stay on the device when nothing on the host reads them: no --profile_out / --ancestral_seqs, no job
    // dump (Backend::resident; PGM_NO_RESIDENT=1 keeps the round trip)
    const bool resident = env.resident_pass;
    LevelState st(L);
    st.tp0 = std::chrono::steady_clock::now();
    if (resident) import_children(a, nodes, owner, level);
    prepare_level(env, nodes, level, st.pend);
    st.tp1 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < L; ++k) st.worker_of[k] = owner[(size_t)level[k]];
    st.ar = align_level(st.pend, resident && default_backend().workers() > 1 ? &st.worker_of : nullptr);
    st.tp2 = std::chrono::steady_clock::now();
    // mergeGraphs of the whole level: plans on host threads, the node profiles in ONE device batch, then edges / Graph /
    // extend_alignment on host threads again
    plan_merges(env, nodes, level, st);
    st.tq0 = std::chrono::steady_clock::now();
    bool on_device = false;
    // (a resident pass: the graphs below need the plans only, not the profiles — the device batch of the node profiles runs on a
    // thread of its own beside them)
    std::thread merge_thread;
    std::exception_ptr merge_error;
    bool all_on_device = true;
    if (!host_switches().host_merge)   // (filled before the thread starts: the graphs section below releases the children)
        for (size_t k = 0; k < L; ++k) {
            const Node &nd = nodes[level[k]];
            const Graph &ga = nodes[nd.child[0]].res.graph, &gb = nodes[nd.child[1]].res.graph;
            pgm_merge_job &j = st.mj[k];
            j.dim = (uint32_t)a.DIM; j.n1 = ga.size(); j.n2 = gb.size(); j.nnodes = (uint32_t)st.plans[k].mapping1.size();
            j.sites1 = ga.devSites() ? ga.devSites() : ga.col(0); j.sites2 = gb.devSites() ? gb.devSites() : gb.col(0);
            j.P1 = st.pend[k].model1.P.data(); j.P2 = st.pend[k].model2.P.data();
            j.k1 = st.plans[k].mapping1.data(); j.k2 = st.plans[k].mapping2.data(); j.g2_with_P1 = st.plans[k].g2_with_P1.data();
            j.profiles = resident ? nullptr : st.profiles[k].data();
            all_on_device = all_on_device && ga.devSites() && gb.devSites();
        }
    auto merge_on_device = [&]() {
        if (host_switches().host_merge) return;
        const auto tm0 = std::chrono::steady_clock::now();
        on_device = merge_profiles_on_device(st, resident);
        default_backend().seconds_merge_profiles += std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count();
    };
    if (resident && all_on_device && !host_switches().host_merge) merge_thread = std::thread([&]() { try { merge_on_device(); } catch (...) { merge_error = std::current_exception(); } });
    else merge_on_device();
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } merge_joiner{merge_thread};   // (also when the section below throws)
    st.tq1 = std::chrono::steady_clock::now();
    finish_nodes(env, nodes, level, st, !resident && !on_device);
    if (merge_thread.joinable()) {
        merge_thread.join();
        if (merge_error) std::rethrow_exception(merge_error);
    }
    if (resident) for (size_t k = 0; k < L; ++k) nodes[level[k]].res.graph.setDevSites(st.dev_profiles[k]);
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
                std::chrono::duration<double, std::milli>(tp3 - env.tl0).count(), h, L,
                std::chrono::duration<double, std::milli>(st.tp1 - st.tp0).count(), std::chrono::duration<double, std::milli>(st.tp2 - st.tp1).count(),
                std::chrono::duration<double, std::milli>(tp3 - st.tp2).count()),
        fprintf(stderr, "    post: plans %.1f ms, node profiles %.1f, edges / graphs / extend %.1f (summed over the nodes: graphs %.2f ms, extend_alignment %.2f)\n", std::chrono::duration<double, std::milli>(st.tq0 - st.tp2).count(),
                std::chrono::duration<double, std::milli>(st.tq1 - st.tq0).count(), std::chrono::duration<double, std::milli>(tp3 - st.tq1).count(), st.ns_merge.load() / 1e6, st.ns_extend.load() / 1e6);
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

    // ---- leaves (ProgressiveAlignment.cpp:17-46) ----
    std::vector<int> leaves;
    std::vector<const sequence_t *> seq_of(nodes.size(), nullptr);   // a leaf's sequence, by node
    for (size_t i = 0; i < nodes.size(); ++i)
        if (nodes[i].tree->isLeaf()) {
            leaves.push_back((int)i);
            seq_of[i] = &families[(size_t)nodes[i].fam].sequences->at(nodes[i].tree->getName());
        }
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
        for (int li : leaves) leaf_len[(size_t)li] = (double)seq_of[(size_t)li]->size();
        owner = assign_owners(nodes, roots[(size_t)nodes[0].fam], default_backend().workers(), leaf_len);
    }
    default_backend().resident_pass = resident_pass;
    default_backend().resident_imports = 0;
    const auto tl1 = std::chrono::steady_clock::now();
    parallel_for(leaves.size(), [&](size_t k) {   // (independent leaves: a thousand SequenceGraphs are 50 ms on one thread)
        Node &nd = nodes[(size_t)leaves[k]];
        const std::string &name = nd.tree->getName();
        init_leaf(a, nd.res, *seq_of[(size_t)leaves[k]], resident_leaves ? LeafGraph::OnDevice : csprofile ? LeafGraph::None : LeafGraph::OnHost, &name);
        if (!resident_leaves && !csprofile && !cmdlineopts.profile_file.empty()) {   // result.profiles[name] = sites without START / END (ProgressiveAlignment.h:73)
            Profile &pf = nd.res.profiles[name];
            pf.dim = a.DIM; pf.cols = nd.res.graph.size() - 2;
            pf.data.assign(nd.res.graph.col(1), nd.res.graph.col(1) + (size_t)a.DIM * pf.cols);
        }
    });
    const auto tl2 = std::chrono::steady_clock::now();
    if (resident_leaves)
        for (int w = 0; w < default_backend().workers(); ++w) {   // every worker builds the leaves of its subtrees
            std::vector<int> mine;
            for (int li : leaves) if (owner[(size_t)li] == w) mine.push_back(li);
            upload_onehot_leaves(a, nodes, mine, seq_of, w);
        }
    if (csprofile) {
        if (forest && cmdlineopts.aafreqs_flag) {
            std::vector<std::vector<int>> of_family(families.size());
            for (int li : leaves) of_family[(size_t)nodes[(size_t)li].fam].push_back(li);
            for (const std::vector<int> &group : of_family) if (!group.empty()) csprofile_leaves(a, *csprofile, fenv, nodes, group, seq_of, resident_pass, owner);
        } else csprofile_leaves(a, *csprofile, fenv, nodes, leaves, seq_of, resident_pass, owner);
    }
    for (int li : leaves) {   // (in the order of the families: `nodes` holds one tree after the other)
        const FamEnv &fe = fenv[(size_t)nodes[(size_t)li].fam];
        if (fe.with_repeats()) attach_repeats(nodes[(size_t)li].res, nodes[(size_t)li].tree->getName(), *fe.repeats);
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

}  // namespace pgm
