// root_search.cpp — the root search -r / -rr (reference src/FindRoot.h, GapParsimony.h).
// The reference memoises one alignment per directed subtree of the unrooted guide tree (node::getAlignment) and one per branch
// (edge::getAlignment), computing them on demand in its recursion.  Here they are the nodes of a DAG of merges, run height by
// height through run_level like the levels of a plain pass.  Rows are not carried through the DAG: every merge keeps its two
// mappings and a gap mask of its rows (one bit per column), which is all the gap parsimony reads; the winner's rows are
// composed from the mappings at the end.
#include "progressive_internal.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <iostream>

namespace pgm {

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
        std::vector<const sequence_t *> seq_of(nodes.size(), nullptr);
        parallel_for(leaves.size(), [&](size_t k) {
            Node &nd = nodes[(size_t)leaves[k]];
            const sequence_t &seq = sequences.at(nd.tree->getName());
            seq_of[(size_t)leaves[k]] = &seq;
            // (the header's tree2graph: plain sequence graphs even with -c, FindRoot.h:183)
            init_leaf(a, nd.res, seq, env.resident_pass ? LeafGraph::OnDevice : LeafGraph::OnHost, nullptr);
            GapMask &m = mask[(size_t)leaves[k]];
            m.ncols = (uint32_t)seq.size();
            m.bits.assign((seq.size() + 63) / 64, 0ull);
            for (size_t c = 0; c < seq.size(); ++c) if (a.isGap(seq[c])) m.bits[c >> 6] |= 1ull << (c & 63);
            done[(size_t)leaves[k]] = 1;
        });
        if (env.resident_pass) upload_onehot_leaves(a, nodes, leaves, seq_of, 0);
        if (env.fams[0].with_repeats())
            for (int li : leaves) attach_repeats(nodes[(size_t)li].res, nodes[(size_t)li].tree->getName(), *env.fams[0].repeats);
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

}  // namespace pgm
