// wls.cpp — the weighted least-squares refinement of a guide tree, -W / -WW (reference src/LeastSquares.cpp, NNLS.h).
// The subtree pair sums of a quartet or quintet go to the backend (pgm_wls_pair_sums_batch; wls_pair_sums_host states the kernels'
// summation order and is the backend's default), the NNLS fits and the rewiring of the tree stay on the host.
#include "pgm_host.h"
#include "nnls.h"
#include <algorithm>
#include <chrono>
#include <cmath>

namespace pgm {
// ---- LeastSquares::refineTree (LeastSquares.cpp) ----------------------------------------------------------------------
// The reference's unrooted node / edge arrays and its pointer rewiring are kept as they are: toTree() roots at edges[0] and
// takes the children in node.edges[] order, which decides the newick text and the tree order of the alignment.  The pair sums
// of OptimizeQuartet / OptimizeQuintet (:305-325, :557-577) go to the backend (one edge per call while a sweep may change the
// tree, every edge in one call for the final support pass); they are added in the kernels' fixed order instead of the
// reference's std::map walk, so they may differ from the reference's in the last bits.  computeFit, which decides when the
// sweeps stop, is restated in the reference's order on the host.
WlsStats wls_stats;

namespace {
const uint32_t WLS_ROWS = 16, WLS_SLOTS = PGM_WLS_OUT;   // = PGM_WLS_ROWS, PGM_WLS_SLOTS of csrc/pgm_wls_kernels.h

// lane 0 of the kernels' xor butterfly (v_t += v_{t^m}, m = 32 .. 1): at step m only the lanes below m still reach lane 0
double wave_sum(double v[64]) {
    for (int m = 32; m >= 1; m >>= 1)
        for (int t = 0; t < m; ++t) v[t] = v[t] + v[t + m];
    return v[0];
}
}  // namespace

void wls_pair_sums_host(uint32_t n, const double *D, const double *W, uint32_t njobs, const pgm_wls_job *jobs, double *out) {
    const uint32_t nblocks = (n + WLS_ROWS - 1) / WLS_ROWS;
    std::vector<double> part((size_t)nblocks * WLS_SLOTS);
    for (uint32_t j = 0; j < njobs; ++j) {
        const int8_t *lab = jobs[j].label;
        const double *off = jobs[j].offset;
        const int K = (int)jobs[j].nsub;
        if (K != 4 && K != 5) error("wls: nsub must be 4 or 5");
        auto block = [&](size_t b) {   // pgm_wls_rows_kernel: wave v takes the rows v, v + 4, ... of the block
            double acc[4][WLS_SLOTS] = {};
            for (uint32_t v = 0; v < 4; ++v)
                for (uint32_t i = 0; i < WLS_ROWS / 4; ++i) {
                    const uint32_t k = (uint32_t)b * WLS_ROWS + v + 4 * i;
                    if (k >= n) break;
                    const int p = lab[k];
                    if (p < 0 || p >= K - 1) continue;
                    double s[4][64] = {}, w[4][64] = {};
                    const double a = off[k];
                    const double *Dk = D + (size_t)k * n, *Wk = W + (size_t)k * n;
                    for (uint32_t l = 0; l < n; ++l) {
                        const int q = lab[l] - p - 1;
                        if (q < 0) continue;
                        s[q][l & 63] += Wk[l] * ((Dk[l] - a) - off[l]);
                        w[q][l & 63] += Wk[l];
                    }
                    const int base = p * K - p * (p + 1) / 2;
                    for (int q = 0; q < K - 1 - p; ++q) {
                        acc[v][base + q] += wave_sum(s[q]);
                        acc[v][10 + base + q] += wave_sum(w[q]);
                    }
                }
            for (uint32_t q = 0; q < WLS_SLOTS; ++q) part[b * WLS_SLOTS + q] = (acc[0][q] + acc[1][q]) + (acc[2][q] + acc[3][q]);
        };
        if (nblocks >= 8) parallel_for(nblocks, block);
        else for (uint32_t b = 0; b < nblocks; ++b) block(b);
        double c[WLS_SLOTS][64] = {};   // pgm_wls_jobs_kernel: lane t adds the blocks t, t + 64, ...
        for (uint32_t b = 0; b < nblocks; ++b)
            for (uint32_t q = 0; q < WLS_SLOTS; ++q) c[q][b & 63] += part[(size_t)b * WLS_SLOTS + q];
        for (uint32_t q = 0; q < WLS_SLOTS; ++q) out[(size_t)j * WLS_SLOTS + q] = wave_sum(c[q]);
    }
}

void Backend::wls_load(uint32_t n, const double *D, const double *W, int) {
    wls_n = n;
    wls_D.assign(D, D + (size_t)n * n);
    wls_W.assign(W, W + (size_t)n * n);
}

void Backend::wls_pair_sums_batch(uint32_t njobs, const pgm_wls_job *jobs, double *out, int) {
    if (wls_n == 0) error("wls: no matrices loaded");
    wls_pair_sums_host(wls_n, wls_D.data(), wls_W.data(), njobs, jobs, out);
}

namespace {
namespace ls {

struct Node;
struct Edge {   // :29-46
    Node *nodes[2];
    distance_t length;
    double support;
    Node &other(const Node &node) const { return *(nodes[0] == &node ? nodes[1] : nodes[0]); }
    Node &operator[](int i) const { return *nodes[i]; }
};
struct Node {   // :48-62
    Edge *edges[3];
    index_t leaf;
    bool todo;
    bool isLeaf() const { return leaf != (index_t)-1; }
    Edge &operator[](int i) const { return *edges[i]; }
};

struct Graph {   // :64-200
    std::vector<Node> nodes;
    std::vector<Edge> edges;
    std::map<std::string, index_t> leaf_of;
    std::vector<std::string> labels;
    index_t n_leaves = 0, n_nodes = 0, n_edges = 0;

    Graph(const PhyTree &tree, const std::vector<std::string> &leaves_order) : labels(leaves_order) {
        if (tree.n_children() != 2) error("wls_refine: the tree's root must have two children");
        n_leaves = (index_t)leaves_order.size();
        nodes.resize(2 * (size_t)n_leaves - 2);
        edges.resize(2 * (size_t)n_leaves - 3);
        for (index_t i = 0; i < n_leaves; ++i) leaf_of.emplace(leaves_order[i], i);
        n_nodes = 0;
        n_edges = 1;
        edges[0].length = tree[0].getBranchLength() + tree[1].getBranchLength();
        edges[0].nodes[0] = tree2graphR(tree[0], &edges[0]);
        edges[0].nodes[1] = tree2graphR(tree[1], &edges[0]);
        if (n_nodes != nodes.size() || n_edges != edges.size()) error("wls_refine: the tree is not binary");
    }
    Node *tree2graphR(const PhyTree &tree, Edge *edge) {
        Node &node = nodes[n_nodes++];
        node.leaf = (index_t)-1;
        node.edges[0] = edge;
        if (tree.isLeaf()) {
            node.edges[1] = node.edges[2] = nullptr;
            auto it = leaf_of.find(tree.getName());
            if (it == leaf_of.end()) error("unknown leaf name: %s", tree.getName().c_str());
            node.leaf = it->second;
        } else {
            if (tree.n_children() != 2) error("wls_refine: the tree is not binary");
            for (int c = 0; c < 2; ++c) {
                node.edges[1 + c] = &edges[n_edges++];
                node[1 + c].length = tree[c].getBranchLength();
                node[1 + c].nodes[0] = &node;
                node[1 + c].nodes[1] = tree2graphR(tree[c], node.edges[1 + c]);
            }
        }
        return &node;
    }
    index_t index(const Node *n) const { return (index_t)(n - nodes.data()); }

    // subtreeDistR (:172-183): every leaf below `node` (away from `from`) with its path length, visited in the reference's order
    template <class F> static void subtreeDistR(const Node *node, const Edge *from, distance_t dist, const F &leaf) {
        if (node->isLeaf()) { leaf(node, dist); return; }
        for (int i = 0; i < 3; ++i) {
            const Edge *e = node->edges[i];
            if (e != from) subtreeDistR(&e->other(*node), e, dist + e->length, leaf);
        }
    }

    PhyTree *toTree() const {   // :117-123
        const Edge &e = edges[0];
        PhyTree *root = new PhyTree();
        root->addChild(toTreeR(&e[0], &e), e.length / 2.0, e.support);
        root->addChild(toTreeR(&e[1], &e), e.length / 2.0, e.support);
        return root;
    }
    PhyTree *toTreeR(const Node *node, const Edge *from) const {   // :185-199
        if (node->isLeaf()) return new PhyTree(labels[node->leaf]);
        PhyTree *tree = new PhyTree();
        for (int i = 0; i < 3; ++i) {
            const Edge *e = node->edges[i];
            if (e != from) tree->addChild(toTreeR(&e->other(*node), e), e->length, e->support);
        }
        return tree;
    }
};

struct Refiner {
    Graph &g;
    const DistanceMatrix &w;   // distances and weights (1 / variance)
    Backend &be;
    uint32_t n;
    std::vector<int8_t> label;
    std::vector<double> offset;

    // computeFit (:202-217): the leaves of subtreeDist's std::map come in node-array order
    double computeFit() {
        double fit = 0.0;
        std::vector<double> dist(g.nodes.size());
        std::vector<char> seen(g.nodes.size());
        for (index_t i = 0; i < g.n_nodes; ++i) {
            const Node &nd = g.nodes[i];
            if (!nd.isLeaf()) continue;
            const index_t i1 = nd.leaf;
            std::fill(seen.begin(), seen.end(), 0);
            Graph::subtreeDistR(&nd[0].other(nd), &nd[0], 0.0, [&](const Node *leaf, distance_t d) {
                const index_t k = g.index(leaf);
                dist[k] = d; seen[k] = 1;
            });
            for (index_t k = 0; k < g.n_nodes; ++k) {
                if (!seen[k]) continue;
                const index_t i2 = g.nodes[k].leaf;
                const double D = w.distances[(size_t)i1 * n + i2], W = w.variances[(size_t)i1 * n + i2];
                fit += (dist[k] + nd[0].length - D) * W * (dist[k] + nd[0].length - D);
            }
        }
        return fit;
    }

    // the labels and offsets of one job: leaf l of subtree i = below nodes[i], away from edges[i]
    void job(int K, Node *const *nodes, Edge *const *edges, int8_t *lab, double *off) {
        std::fill(lab, lab + n, (int8_t)-1);
        std::fill(off, off + n, 0.0);
        for (int i = 0; i < K; ++i)
            Graph::subtreeDistR(nodes[i], edges[i], 0.0, [&](const Node *leaf, distance_t d) { lab[leaf->leaf] = (int8_t)i; off[leaf->leaf] = d; });
    }
    void pair_sums(uint32_t njobs, const pgm_wls_job *jobs, double *out) {
        const auto t0 = std::chrono::steady_clock::now();
        be.wls_pair_sums_batch(njobs, jobs, out);
        wls_stats.pair_sums_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        ++wls_stats.batches;
    }
    // the aggregated K x K matrix (:326-327): distances = sums / sqrt(weights)
    static void aggregate(int K, const double *sums, double *Dk, double *Wk) {
        int s = 0;
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j, ++s) {
                Wk[i * K + j] = Wk[j * K + i] = std::sqrt(sums[10 + s]);
                Dk[i * K + j] = Dk[j * K + i] = sums[s] / Wk[i * K + j];
            }
    }
};

// The design matrices of Opt4 (:220-226), Opt5v1 (:353-363) and Opt5v2 (:440-450): one row per pair of subtrees in
// lexicographic order, as bit masks of the edges on the pair's path (bit c = column c; columns 0..K-1 are the subtrees'
// own edges, the rest the inner edges).
const uint8_t ROWS4[6] = {0x03, 0x15, 0x19, 0x16, 0x1A, 0x0C};
const uint8_t ROWS5V1[10] = {0x03, 0x25, 0x29, 0x11, 0x26, 0x2A, 0x52, 0x0C, 0x74, 0x78};
const uint8_t ROWS5V2[10] = {0x03, 0x65, 0x69, 0x31, 0x66, 0x6A, 0x32, 0x0C, 0x54, 0x58};

// the fit of one topology (the NNLS of Opt4 / Opt5v*): new_dists and |A new_dists - dists|^2
double fitTopology(int K, const uint8_t *rows, const index_t *lm, const double *Dk, const double *Wk, double *new_dists) {
    const int R = K * (K - 1) / 2, C = 2 * K - 3;
    double dists[10], weights[10], A[10 * 7];
    int r = 0;
    for (int i = 0; i < K; ++i)
        for (int j = i + 1; j < K; ++j, ++r) {
            dists[r] = Dk[lm[i] * K + lm[j]];
            weights[r] = Wk[lm[i] * K + lm[j]];
        }
    for (r = 0; r < R; ++r)
        for (int c = 0; c < C; ++c) A[r * C + c] = weights[r] * (double)((rows[r] >> c) & 1);
    nnls::solve(R, C, A, dists, new_dists);
    double fit = 0;
    for (r = 0; r < R; ++r) {
        double ax = 0;
        for (int c = 0; c < C; ++c) ax += A[r * C + c] * new_dists[c];
        fit += (ax - dists[r]) * (ax - dists[r]);
    }
    return fit;
}

double Opt4(const index_t lm[4], Node *nodes[6], Edge *edges[5], const double *Dk, const double *Wk, double &best_fit, bool apply) {   // :219-279
    double x[5];
    const double fit = fitTopology(4, ROWS4, lm, Dk, Wk, x);
    if (fit < best_fit && apply) {
        best_fit = fit;
        for (int i = 0; i < 4; ++i) {
            edges[lm[i]]->length = x[i];
            edges[lm[i]]->nodes[0] = nodes[lm[i]];
        }
        edges[4]->length = x[4];
        edges[4]->nodes[0] = nodes[4];
        edges[4]->nodes[1] = nodes[5];
        nodes[4]->edges[0] = edges[4];
        nodes[4]->edges[1] = edges[lm[0]];
        nodes[4]->edges[2] = edges[lm[1]];
        nodes[5]->edges[0] = edges[4];
        nodes[5]->edges[1] = edges[lm[2]];
        nodes[5]->edges[2] = edges[lm[3]];
        edges[lm[0]]->nodes[1] = nodes[4];
        edges[lm[1]]->nodes[1] = nodes[4];
        edges[lm[2]]->nodes[1] = nodes[5];
        edges[lm[3]]->nodes[1] = nodes[5];
    }
    return fit;
}

double Opt5(bool v2, const index_t lm[5], Node *nodes[8], Edge *edges[7], const double *Dk, const double *Wk, double &best_fit, bool apply) {   // :351-523
    double x[7];
    const double fit = fitTopology(5, v2 ? ROWS5V2 : ROWS5V1, lm, Dk, Wk, x);
    if (fit < best_fit && apply) {
        best_fit = fit;
        for (int i = 0; i < 5; ++i) {
            edges[lm[i]]->length = x[i];
            edges[lm[i]]->nodes[0] = nodes[lm[i]];
        }
        edges[5]->length = x[5];
        edges[6]->length = x[6];
        if (!v2) {   // Opt5v1: node 4 at the branch to 0
            edges[5]->nodes[0] = nodes[5]; edges[5]->nodes[1] = nodes[6];
            edges[6]->nodes[0] = nodes[5]; edges[6]->nodes[1] = nodes[7];
            nodes[5]->edges[0] = edges[5]; nodes[5]->edges[1] = edges[6]; nodes[5]->edges[2] = edges[lm[1]];
            nodes[6]->edges[0] = edges[5]; nodes[6]->edges[1] = edges[lm[2]]; nodes[6]->edges[2] = edges[lm[3]];
            nodes[7]->edges[0] = edges[6]; nodes[7]->edges[1] = edges[lm[0]]; nodes[7]->edges[2] = edges[lm[4]];
            edges[lm[0]]->nodes[1] = nodes[7];
            edges[lm[1]]->nodes[1] = nodes[5];
            edges[lm[2]]->nodes[1] = nodes[6];
            edges[lm[3]]->nodes[1] = nodes[6];
            edges[lm[4]]->nodes[1] = nodes[7];
            nodes[5]->todo = true; nodes[6]->todo = true; nodes[7]->todo = true;
        } else {     // Opt5v2: node 4 in the centre
            edges[5]->nodes[0] = nodes[5]; edges[5]->nodes[1] = nodes[7];
            edges[6]->nodes[0] = nodes[6]; edges[6]->nodes[1] = nodes[7];
            nodes[5]->edges[0] = edges[5]; nodes[5]->edges[1] = edges[lm[0]]; nodes[5]->edges[2] = edges[lm[1]];
            nodes[6]->edges[0] = edges[6]; nodes[6]->edges[1] = edges[lm[2]]; nodes[6]->edges[2] = edges[lm[3]];
            nodes[7]->edges[0] = edges[5]; nodes[7]->edges[1] = edges[6]; nodes[7]->edges[2] = edges[lm[4]];
            edges[lm[0]]->nodes[1] = nodes[5];
            edges[lm[1]]->nodes[1] = nodes[5];
            edges[lm[2]]->nodes[1] = nodes[6];
            edges[lm[3]]->nodes[1] = nodes[6];
            edges[lm[4]]->nodes[1] = nodes[7];
            nodes[5]->todo = true; nodes[6]->todo = true; nodes[7]->todo = false;
        }
    }
    return fit;
}

// OptimizeQuartet (:281-339) around an inner edge: the four subtrees; false for an edge to a leaf
bool quartetAround(Edge *e, Node *nodes[6], Edge *edges[5]) {
    if ((*e)[0].isLeaf() || (*e)[1].isLeaf()) return false;
    edges[4] = e;
    nodes[4] = &(*e)[0];
    nodes[5] = &(*e)[1];
    edges[0] = &(*nodes[4])[0] == e ? &(*nodes[4])[1] : &(*nodes[4])[0];
    edges[1] = &(*nodes[4])[2] == e ? &(*nodes[4])[1] : &(*nodes[4])[2];
    edges[2] = &(*nodes[5])[0] == e ? &(*nodes[5])[1] : &(*nodes[5])[0];
    edges[3] = &(*nodes[5])[2] == e ? &(*nodes[5])[1] : &(*nodes[5])[2];
    nodes[0] = &edges[0]->other(*nodes[4]);
    nodes[1] = &edges[1]->other(*nodes[4]);
    nodes[2] = &edges[2]->other(*nodes[5]);
    nodes[3] = &edges[3]->other(*nodes[5]);
    return true;
}
double quartetSupport(Edge *e, Node *nodes[6], Edge *edges[5], const double *sums, bool apply) {
    double Dk[16], Wk[16], best_fit = INFINITY;
    Refiner::aggregate(4, sums, Dk, Wk);
    static const index_t m1[4] = {0, 1, 2, 3}, m2[4] = {0, 2, 1, 3}, m3[4] = {0, 3, 1, 2};
    const double f1 = Opt4(m1, nodes, edges, Dk, Wk, best_fit, apply);
    const double f2 = Opt4(m2, nodes, edges, Dk, Wk, best_fit, apply);
    const double f3 = Opt4(m3, nodes, edges, Dk, Wk, best_fit, apply);
    return e->support = 1.0 / (1.0 + std::exp((f2 - f1) / -2.0) + std::exp((f3 - f1) / -2.0));
}

// OptimizeQuartets (:341-348).  apply == false (the support pass) cannot change the tree: every inner edge in one batch.
void OptimizeQuartets(Refiner &R, bool apply) {
    Graph &g = R.g;
    Node *nodes[6];
    Edge *edges[5];
    double sums[PGM_WLS_OUT];
    if (apply) {
        for (index_t i = 0; i < g.n_edges; ++i) {
            Edge *e = &g.edges[i];
            if (!quartetAround(e, nodes, edges)) { e->support = edge_support(e->length); continue; }
            R.job(4, nodes, edges, R.label.data(), R.offset.data());
            const pgm_wls_job j = {R.label.data(), R.offset.data(), 4};
            R.pair_sums(1, &j, sums);
            ++wls_stats.quartets;
            quartetSupport(e, nodes, edges, sums, true);
        }
        return;
    }
    std::vector<index_t> inner;
    for (index_t i = 0; i < g.n_edges; ++i) {
        if (quartetAround(&g.edges[i], nodes, edges)) inner.push_back(i);
        else g.edges[i].support = edge_support(g.edges[i].length);
    }
    if (inner.empty()) return;
    std::vector<int8_t> lab((size_t)inner.size() * R.n);
    std::vector<double> off((size_t)inner.size() * R.n), out((size_t)inner.size() * PGM_WLS_OUT);
    std::vector<pgm_wls_job> jobs(inner.size());
    for (size_t k = 0; k < inner.size(); ++k) {
        quartetAround(&g.edges[inner[k]], nodes, edges);
        R.job(4, nodes, edges, lab.data() + k * R.n, off.data() + k * R.n);
        jobs[k] = pgm_wls_job{lab.data() + k * R.n, off.data() + k * R.n, 4};
    }
    R.pair_sums((uint32_t)jobs.size(), jobs.data(), out.data());
    wls_stats.quartets += inner.size();
    for (size_t k = 0; k < inner.size(); ++k) {
        Edge *e = &g.edges[inner[k]];
        quartetAround(e, nodes, edges);
        quartetSupport(e, nodes, edges, out.data() + k * PGM_WLS_OUT, false);
    }
}

// OptimizeQuintet (:525-629): centre node n, edge e to node 4
bool OptimizeQuintet(Refiner &R, Node *n, Edge *e, bool apply) {
    double best_fit = INFINITY;
    Node *nodes[8];
    Edge *edges[7];
    edges[4] = e;
    nodes[7] = n;
    nodes[4] = &edges[4]->other(*n);
    if (nodes[7]->isLeaf()) return false;
    edges[5] = &(*nodes[7])[0] == e ? &(*nodes[7])[1] : &(*nodes[7])[0];
    edges[6] = &(*nodes[7])[2] == e ? &(*nodes[7])[1] : &(*nodes[7])[2];
    nodes[5] = &edges[5]->other(*nodes[7]);
    nodes[6] = &edges[6]->other(*nodes[7]);
    if (nodes[5]->isLeaf() || nodes[6]->isLeaf()) return false;
    edges[0] = &(*nodes[5])[0] == edges[5] ? &(*nodes[5])[1] : &(*nodes[5])[0];
    edges[1] = &(*nodes[5])[2] == edges[5] ? &(*nodes[5])[1] : &(*nodes[5])[2];
    edges[2] = &(*nodes[6])[0] == edges[6] ? &(*nodes[6])[1] : &(*nodes[6])[0];
    edges[3] = &(*nodes[6])[2] == edges[6] ? &(*nodes[6])[1] : &(*nodes[6])[2];
    nodes[0] = &edges[0]->other(*nodes[5]);
    nodes[1] = &edges[1]->other(*nodes[5]);
    nodes[2] = &edges[2]->other(*nodes[6]);
    nodes[3] = &edges[3]->other(*nodes[6]);

    R.job(5, nodes, edges, R.label.data(), R.offset.data());
    const pgm_wls_job j = {R.label.data(), R.offset.data(), 5};
    double sums[PGM_WLS_OUT], Dk[25], Wk[25];
    R.pair_sums(1, &j, sums);
    ++wls_stats.quintets;
    Refiner::aggregate(5, sums, Dk, Wk);
    // (:581-626) per split of the four outer subtrees: Opt5v2 with 4 in the centre, then Opt5v1 with 4 at each outer branch
    static const index_t maps[15][5] = {
        {0, 1, 2, 3, 4}, {0, 1, 2, 3, 4}, {1, 0, 2, 3, 4}, {2, 3, 0, 1, 4}, {3, 2, 0, 1, 4},
        {0, 2, 1, 3, 4}, {0, 2, 1, 3, 4}, {2, 0, 1, 3, 4}, {1, 3, 0, 2, 4}, {3, 1, 0, 2, 4},
        {0, 3, 1, 2, 4}, {0, 3, 1, 2, 4}, {3, 0, 1, 2, 4}, {1, 2, 0, 3, 4}, {2, 1, 0, 3, 4}};
    double f1 = 0;
    for (int m = 0; m < 15; ++m) {
        const double f = Opt5(m % 5 == 0, maps[m], nodes, edges, Dk, Wk, best_fit, apply);
        if (m == 0) f1 = f;
    }
    return best_fit < f1;
}

void OptimizeQuintets(Refiner &R, bool apply) {   // :631-658
    Graph &g = R.g;
    for (index_t i = 0; i < g.n_nodes; ++i) g.nodes[i].todo = true;
    for (int k = 0; k < 5; ++k) {   // MAX_ITERS5
        bool any = false;
        for (index_t i = 0; i < g.n_nodes; ++i) {
            Node *nd = &g.nodes[i];
            if (!nd->todo) continue;
            nd->todo = false;
            if (nd->isLeaf()) continue;
            for (int j = 0; j < 3; ++j)
                if (OptimizeQuintet(R, nd, nd->edges[j], apply)) { any = true; break; }
        }
        if (!any) break;
    }
}

}  // namespace ls
}  // namespace

PhyTree *refineTree(PhyTree *tree, const std::vector<std::string> &leaf_order, const DistanceMatrix &dist) {   // :661-710
    const auto t0 = std::chrono::steady_clock::now();
    ls::Graph g(*tree, leaf_order);
    const uint32_t n = (uint32_t)leaf_order.size();
    DistanceMatrix weights = dist;
    for (double &v : weights.variances) v = 1.0 / v;
    Backend &be = default_backend();
    be.wls_load(n, weights.distances.data(), weights.variances.data());
    ls::Refiner R{g, weights, be, n, std::vector<int8_t>(n), std::vector<double>(n)};
    ++wls_stats.trees;

    double fit1 = R.computeFit();
    ls::OptimizeQuartets(R, true);
    double fit2 = R.computeFit();
    ++wls_stats.sweeps;
    int i = 0;
    do {
        fit1 = fit2;
        if (cmdlineopts.wlsrefine_flag > 1) {
            ls::OptimizeQuintets(R, true);
            fit2 = R.computeFit();
        }
        ls::OptimizeQuartets(R, true);
        fit2 = R.computeFit();
        ++wls_stats.sweeps;
        ++i;
    } while (fit2 < fit1 && i < 20);   // MAX_ITERS
    ls::OptimizeQuartets(R, false);   // the supports only

    delete tree;
    tree = g.toTree();
    wls_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return tree;
}
}  // namespace pgm
