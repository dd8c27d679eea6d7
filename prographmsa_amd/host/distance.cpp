// distance.cpp — pairwise distances and the BioNJ guide tree for the `-a` path
// (reference src/DistanceFactoryAlign.{h,cpp}, DistanceFactoryML.{h,cpp}, TreeNJ.{h,cpp}).
// The O(L^2) Needleman-Wunsch of every pair (alignPair), the pair counts of an alignment and the k-mer cosine matrix run behind the
// C ABI, and so does ML distance estimation when PGM_DEVICE_MLDIST is set (pgm_mldist_batch; on the host threads otherwise);
// the joins of neighbour joining run on the host threads or, from kBionjDeviceMin taxa on, behind pgm_bionj_multi; with a fixed topology (--topology) the pairs come from a plan.  TreeNJ (one family) and TreeNJ_multi (--batch) are one implementation: the last section.
#include "pgm_host.h"
#include "nnls.h"
#include <quadmath.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <fstream>
#include <functional>
#include <thread>

namespace pgm {

// ---- DistanceFactoryML ---------------------------------------------------------------------
static void consts(const Alphabet &a, double &DIST_MAX, double &VAR_MAX, double &VAR_MIN) {  // DistanceFactoryML.cpp:5-32
    if (a.kind == ALPHA_AA || a.kind == ALPHA_DNA) { DIST_MAX = 2.2; VAR_MAX = 1e3; VAR_MIN = 1e-5; }
    else { DIST_MAX = 5.2; VAR_MAX = 5e3; VAR_MIN = 1e-5; }
}

static void matmul(const std::vector<double> &A, const std::vector<double> &B, int n, std::vector<double> &C) {
    C.assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) {
            double b = B[k + n * j];
            for (int i = 0; i < n; ++i) C[i + n * j] += A[i + n * k] * b;
        }
}

distvar_t DistanceFactoryML::computeMLDist(const std::vector<int32_t> &counts, index_t gaps, double seqlen, double dist0,
                                           double var0) const {  // DistanceFactoryML.h:66-135
    const int n = alphabet.DIM;
    double DIST_MAX, VAR_MAX, VAR_MIN;
    consts(alphabet, DIST_MAX, VAR_MAX, VAR_MIN);
    const double EPSILON = 1e-5;
    const index_t MAXITER = 20;
    double dist_min = 0, dist_max = INFINITY;
    double dist = dist0, var = var0;
    double delta = 1;
    index_t iteration = 0;
    std::vector<double> pp, ppp;
    while (std::abs(delta) > EPSILON) {
        if (iteration > MAXITER) {
            if (dist_max == INFINITY) { dist = DIST_MAX; var = VAR_MAX; }
            else { dist = dist0; var = var0; }
            break;
        }
        Model model = model_factory->getModel(dist);
        const std::vector<double> &p = model.P;
        matmul(model.Q, p, n, pp);
        matmul(model.Q, pp, n, ppp);
        double f = 0, ff = 0;
        for (size_t i = 0; i < p.size(); ++i) {
            double c = counts[i];
            f += c * pp[i] / p[i];
            ff += (c * (ppp[i] * p[i] - pp[i] * pp[i])) / (p[i] * p[i]);
        }
        if (cmdlineopts.mldist_gap_flag) {
            double grate = cmdlineopts.indel_rate * seqlen * dist;
            f += (-grate + gaps) / dist;
            ff += -(double)gaps / (dist * dist);
        }
        var = -1.0 / ff;
        if (f > 0) dist_min = std::max(dist_min, dist);
        else dist_max = std::min(dist_max, dist);
        double new_dist = dist - f / ff;
        if (!(new_dist < dist_max && new_dist > dist_min)) {
            double upper = (dist_max == INFINITY) ? dist * 3 : dist_max;
            new_dist = (upper + dist_min) / 2.0;
        }
        delta = 1.0 - new_dist / dist;
        dist = new_dist;
        ++iteration;
    }
    return distvar_t{dist, var};
}

distvar_t DistanceFactoryML::computeDistance(const std::vector<int32_t> &counts, index_t gaps, double seqlen) const {
    const int n = alphabet.DIM;  // DistanceFactoryML.h:137-190
    double DIST_MAX, VAR_MAX, VAR_MIN;
    consts(alphabet, DIST_MAX, VAR_MAX, VAR_MIN);
    double ident = 0, total = 0;
    for (int i = 0; i < n; ++i) ident += counts[i + n * i];
    for (int32_t c : counts) total += c;
    return computeDistance(ident, total, &counts, gaps, seqlen);
}

// (ident, total) are sums of integers, exact in any order: the all-pairs stage reduces them on the device when nothing else of the
// count matrix is read (no --mldist: counts == nullptr)
distvar_t DistanceFactoryML::computeDistance(double ident, double total, const std::vector<int32_t> *counts, index_t gaps, double seqlen) const {
    double DIST_MAX, VAR_MAX, VAR_MIN;
    consts(alphabet, DIST_MAX, VAR_MAX, VAR_MIN);
    double dist0 = 1.0 - ident / total;
    double dist, var;
    if (cmdlineopts.mldist_flag || cmdlineopts.mldist_gap_flag) {
        if (total == 0 || dist0 > 0.85) { dist = dist0 = DIST_MAX; var = VAR_MAX; }
        else { dist = dist0 = -std::log(1.0 - dist0 - 0.2 * dist0 * dist0); var = dist / total; }
        if (total > 0 && ident != total) {
            if (!counts) error("computeDistance: the ML estimate needs the count matrix");
            distvar_t dv = computeMLDist(*counts, gaps, seqlen, dist, var);
            dist = dv.dist;
            var = dv.var;
        }
    } else {
        if (total == 0) { dist = dist0 = 1.0; var = VAR_MAX; }
        else { dist = dist0; var = dist0 / total; }
    }
    if (!(dist < DIST_MAX)) { dist = DIST_MAX; var = VAR_MAX; }
    if (dist > cmdlineopts.cutoff_dist) dist = cmdlineopts.cutoff_dist;
    if (var < VAR_MIN) var = VAR_MIN;
    if (!(var < VAR_MAX)) var = VAR_MAX;
    return distvar_t{dist, var};
}

static std::string g_dist_dump;
void set_dist_dump(const std::string &path) { g_dist_dump = path; }
static void dump_distances(const DistanceMatrix &d) {
    if (g_dist_dump.empty()) return;
    std::ofstream f(g_dist_dump.c_str(), std::ios::binary | std::ios::app);
    const int32_t n = d.dim;
    f.write((const char *)&n, 4);
    f.write((const char *)d.distances.data(), 8 * d.distances.size());
    f.write((const char *)d.variances.data(), 8 * d.variances.size());
}

static std::string g_joins_dump;
void set_joins_dump(const std::string &path) { g_joins_dump = path; }
static void dump_joins(int32_t n, const std::vector<pgm_bionj_join> &joins, const double *final_d) {
    if (g_joins_dump.empty()) return;
    std::ofstream f(g_joins_dump.c_str(), std::ios::binary | std::ios::app);
    f.write((const char *)&n, 4);
    for (const pgm_bionj_join &j : joins) {
        const int32_t idx[2] = {(int32_t)j.index1, (int32_t)j.index2};
        const double d[2] = {j.dist1, j.dist2};
        f.write((const char *)idx, 8);
        f.write((const char *)d, 16);
    }
    f.write((const char *)final_d, 8 * 9);
}

// ---- DistanceFactoryAlign ---------------------------------------------------------------------
DistanceFactoryAlign::DistanceFactoryAlign(const Alphabet &a, const ModelFactory *mf) : DistanceFactoryML(a, mf) {
    const int sd = a.DIM + 1;  // initMatrix (DistanceFactoryAlign.cpp:5-35, 38-235, 238-249)
    if (a.kind == ALPHA_DNA) {
        // transition / transversion scores over {T, C, A, G, X}: a match +1, a transition (T-C, A-G) -1, a transversion -2,
        // anything against X 0
        scoring_matrix_.resize((size_t)sd * sd);
        for (int i = 0; i < sd; ++i)
            for (int j = 0; j < sd; ++j)
                scoring_matrix_[(size_t)i + (size_t)sd * j] = (i == 4 || j == 4) ? 0 : i == j ? 1 : (i / 2 == j / 2) ? -1 : -2;
        gap_open = -5;
        gap_extend = -2;
        return;
    }
    std::string file = data_dir() + (a.kind == ALPHA_AA ? "/nw_aa.imat" : "/nw_codon.imat");
    std::ifstream in(file.c_str());
    int r = 0, c = 0;
    in >> r >> c;
    if (!in || r != sd || c != sd) error("cannot read NW scoring matrix %s", file.c_str());
    scoring_matrix_.resize((size_t)sd * sd);
    for (int32_t &v : scoring_matrix_) in >> v;
    gap_open = -10;
    gap_extend = -2;
}

// ---- BioNJ (TreeNJ.cpp:22-29, 132-281; the plan of a fixed topology: TreeNJ.cpp:31-130) -------------
static double support(double d) {
    double s = 1.0 - std::exp(-std::log(2.0) * d / cmdlineopts.edge_halflife);
    s = std::min(1.0, std::max(0.0, s));
    if (std::isnan(s)) s = 0.0;
    return s;
}

// Column sum in the association Eigen's vectorised reduction uses for `distances.colwise().sum()` (TreeNJ.cpp:157):
// SSE2 packets of two doubles starting at the first 16-byte aligned element of the column (the matrix is column-major and
// 16-byte aligned, so column j starts aligned iff j*dim is even), two packet accumulators over alternating packets, the
// accumulators added, an odd last packet added, the two lanes added, then the unaligned head and the tail element.
// It matters: when four clusters are left the criterion has the exact tie Q(0,1) = Q(2,3), and the last bit of these sums
// decides which pair is joined, i.e. where the guide tree is rooted (tests/golden: c1.nw_ml.tree, t9.nw_p.tree, t13.nw_p.tree).
// The matrix is not rebuilt after a join (the reference's reduce() copies dim^2 doubles twice per join): it stays in its
// n0 x n0 storage and `act` lists the rows / columns still in it, in the order of the reduced matrix.  The matrix need not be
// symmetric in its last bits (the k-mer angle distances are not, see angleDistances) and BioNJ reads it by rows, by columns and
// at (index1, index2) as well as (index2, index1): a transposed copy keeps the column reads of the sums and of the criterion
// on contiguous memory.
static double eigen_column_sum(const std::vector<double> &tr, size_t ld, const std::vector<int> &act, int n, int j) {
    const double *col = &tr[(size_t)act[(size_t)j] * ld];   // column act[j] of the distances: a row of their transpose
    auto at = [&](int i) { return col[(size_t)act[(size_t)i]]; };
    const int start = std::min<int>(((size_t)j * n) & 1, n);
    const int end2 = start + ((n - start) / 4) * 4, end = start + ((n - start) / 2) * 2;
    if (end == start) {
        double res = at(0);
        for (int k = 1; k < n; ++k) res += at(k);
        return res;
    }
    double a0 = at(start), a1 = at(start + 1);
    if (end - start > 2) {
        double b0 = at(start + 2), b1 = at(start + 3);
        for (int k = start + 4; k < end2; k += 4) { a0 += at(k); a1 += at(k + 1); b0 += at(k + 2); b1 += at(k + 3); }
        a0 += b0; a1 += b1;
        if (end > end2) { a0 += at(end2); a1 += at(end2 + 1); }
    }
    double res = a0 + a1;
    for (int k = 0; k < start; ++k) res += at(k);
    for (int k = end; k < n; ++k) res += at(k);
    return res;
}

// The joins a fixed topology prescribes (TreeNJ.cpp:31-130), in reduced indices with index1 < index2: a node of `topo` is
// visited when all its children have been (a leaf needs no visit), first in, first out; the visit joins the clusters of its
// two children, the joined cluster keeps the smaller index and every index above the larger one moves down by one.  The order
// of the visits shows in the branch lengths, so it has to be the reference's: its work list starts with the nodes all of
// whose children are leaves in the order of a std::map keyed by node address, and its parser allocates a node before its
// children, which makes that the pre-order of the file (tests/golden/topology.json pins it).  A leaf that is no sequence of
// the family has no cluster: a node with one such child passes the other child's cluster up, without a join.  One pair per
// internal node with sequences below both children: seqs_order.size() - 1 pairs, of which the join loop uses all but the
// last two (it stops at three clusters).
// Errors: a sequence that no leaf names (the reference's message, its missing blank included); a sequence that two leaves
// name; a node whose number of children is not two (the reference asserts, and its release build goes on undefined).
std::vector<pgm_bionj_pair> build_topo_plan(const std::vector<std::string> &seqs_order, const PhyTree *topo) {
    const uint32_t NONE = 0xFFFFFFFFu;
    struct Node { const PhyTree *tree; int parent, kid[2]; uint32_t cluster, ready; };   // cluster: reduced index, NONE: no sequence below
    std::vector<Node> nodes;   // in pre-order
    struct Todo { const PhyTree *tree; int parent; index_t slot; };
    std::vector<Todo> todo{Todo{topo, -1, 0}};   // (an explicit stack: a ladder is as deep as it has leaves)
    while (!todo.empty()) {
        const Todo t = todo.back();
        todo.pop_back();
        const int me = (int)nodes.size();
        nodes.push_back(Node{t.tree, t.parent, {-1, -1}, NONE, 0});
        if (t.parent >= 0) {
            if (t.slot < 2) nodes[(size_t)t.parent].kid[t.slot] = me;
            if (t.tree->isLeaf()) ++nodes[(size_t)t.parent].ready;
        }
        for (index_t c = t.tree->n_children(); c-- > 0;) todo.push_back(Todo{&(*t.tree)[(int)c], me, c});   // (the first child on top)
    }
    std::map<std::string, uint32_t> orig_leaf_index;
    for (size_t i = 0; i < seqs_order.size(); ++i) orig_leaf_index[seqs_order[i]] = (uint32_t)i;
    std::vector<int> at(seqs_order.size(), -1);   // reduced index -> the node that holds the cluster
    for (size_t k = 0; k < nodes.size(); ++k) {
        if (!nodes[k].tree->isLeaf()) continue;
        auto pos = orig_leaf_index.find(nodes[k].tree->getName());
        if (pos == orig_leaf_index.end()) continue;
        if (at[pos->second] >= 0) error("sequence \"%s\" appears more than once in given topology", pos->first.c_str());
        at[pos->second] = (int)k;
        nodes[k].cluster = pos->second;
    }
    for (size_t i = 0; i < at.size(); ++i)
        if (at[i] < 0) error("sequence \"%s\"is missing in given topology", seqs_order[i].c_str());
    for (const Node &nd : nodes)
        if (!nd.tree->isLeaf() && nd.tree->n_children() != 2)
            error("--topology: a node with %d children (every node of the topology must have two)", (int)nd.tree->n_children());
    std::vector<int> worklist;   // (a queue: `head` is its front)
    for (size_t k = 0; k < nodes.size(); ++k)
        if (!nodes[k].tree->isLeaf() && nodes[k].ready == 2) worklist.push_back((int)k);
    std::vector<pgm_bionj_pair> plan;
    for (size_t head = 0; head < worklist.size(); ++head) {
        Node &node = nodes[(size_t)worklist[head]];
        uint32_t index1 = nodes[(size_t)node.kid[0]].cluster, index2 = nodes[(size_t)node.kid[1]].cluster;
        if (index1 == NONE || index2 == NONE) {
            node.cluster = index1 == NONE ? index2 : index1;
        } else {
            if (index1 > index2) std::swap(index1, index2);
            plan.push_back(pgm_bionj_pair{index1, index2});
            node.cluster = index1;
            at.erase(at.begin() + (std::ptrdiff_t)index2);
            for (size_t i = index2; i < at.size(); ++i) nodes[(size_t)at[i]].cluster = (uint32_t)i;
        }
        if (node.cluster != NONE) at[node.cluster] = worklist[head];
        if (node.parent >= 0 && ++nodes[(size_t)node.parent].ready == 2) worklist.push_back(node.parent);
    }
    return plan;
}

// O(N^2) per join, N - 3 joins.  What the reference does per join — clamp every entry, column sums, the scan of the criterion, a
// copy of the matrix without the joined column — is here: the clamp of the entries the previous join wrote (the others were
// clamped when they were written, and nothing reads an entry between its join and the next clamp), sums and scan on the host
// threads from 512 clusters on (ranges of columns; the scan keeps the FIRST minimum in column-major order like Eigen's
// minCoeff: a range keeps its first, the ranges are combined in order with the same strict comparison), and no copy.
// The loop records its joins (reduced indices, index1 < index2, and the two branch lengths) and, when it ends, the D of the
// clusters left (final_d: 3 x 3 row-major; for n0 < 4 the matrix as it came, nothing clamped): all bionj_tree needs to assemble
// the tree, and what pgm_bionj_multi computes on the device (same bits: DESIGN.md 3.11).
// With a plan (build_topo_plan; TreeNJ.cpp:158-179) a join takes its pair from it while it has entries: the two column sums of
// that pair, no scan, O(N) per join; everything after the choice of the pair is the same lines (pgm_bionj_plan_multi on the
// device: DESIGN.md 3.12).
void bionj_joins_host(DistanceMatrix dist, std::vector<pgm_bionj_join> &joins, double *final_d, const std::vector<pgm_bionj_pair> *plan) {
    const double MIN_DIST = 1e-4, MIN_VAR = 1e-5;
    const int n0 = dist.dim;
    joins.clear();
    std::vector<int> act((size_t)n0);
    for (int i = 0; i < n0; ++i) act[(size_t)i] = i;
    auto D = [&](int i, int j) -> double & { return dist.D(act[(size_t)i], act[(size_t)j]); };   // (reduced indices)
    auto V = [&](int i, int j) -> double & { return dist.V(act[(size_t)i], act[(size_t)j]); };
    int fresh = -1;   // reduced index of the row / column the previous join wrote (not clamped yet); -1: the whole matrix is new
    std::vector<double> sums;
    const size_t ld = (size_t)n0;
    std::vector<double> tr((size_t)n0 * n0);   // tr[j ld + i] = dist.D(i, j)
    auto T = [&](int i, int j) -> double & { return tr[(size_t)act[(size_t)j] * ld + (size_t)act[(size_t)i]]; };   // the same element as D(i, j)
    for (int dim = n0; dim > 3; --dim) {
        if (fresh < 0) {
            for (double &d : dist.distances) d = std::max(d, MIN_DIST);
            for (double &v : dist.variances) v = std::max(v, MIN_VAR);
            for (int i = 0; i < dim; ++i) { D(i, i) = 0; V(i, i) = 0; }
            for (int i = 0; i < n0; ++i)
                for (int j = 0; j < n0; ++j) tr[(size_t)j * ld + (size_t)i] = dist.distances[(size_t)i * ld + (size_t)j];
        } else {
            for (int i = 0; i < dim; ++i) {   // (the entries a join writes are symmetric)
                if (i == fresh) continue;
                D(fresh, i) = D(i, fresh) = T(fresh, i) = T(i, fresh) = std::max(D(i, fresh), MIN_DIST);
                V(fresh, i) = V(i, fresh) = std::max(V(i, fresh), MIN_VAR);
            }
        }
        sums.assign((size_t)dim, 0.0);  // colwise sums
        int index1 = 0, index2 = 0;
        const size_t step = (size_t)(n0 - dim);
        if (plan && step < plan->size()) {   // the pair is given: its two sums, the bits of the full loop's
            index1 = (int)(*plan)[step].index1; index2 = (int)(*plan)[step].index2;
            if (index1 < 0 || index1 >= index2 || index2 >= dim) error("BioNJ: join %zu of the topology's plan is out of range", step);
            sums[(size_t)index1] = eigen_column_sum(tr, ld, act, dim, index1);
            sums[(size_t)index2] = eigen_column_sum(tr, ld, act, dim, index2);
        } else {
            const bool threads = dim >= 512;   // (a section of half a millisecond and more; tests/test_oracle_golden.py: the 1024-taxon tree)
            const size_t nranges = threads ? 16 : 1;
            auto range = [&](size_t r, int &c0, int &c1) { c0 = (int)((size_t)dim * r / nranges); c1 = (int)((size_t)dim * (r + 1) / nranges); };
            auto sum_range = [&](size_t r) { int c0, c1; range(r, c0, c1); for (int j = c0; j < c1; ++j) sums[(size_t)j] = eigen_column_sum(tr, ld, act, dim, j); };
            if (threads) parallel_for(nranges, sum_range); else sum_range(0);
            // Q = 0.5 d - 0.5/(dim-2) (S + S^T); minCoeff scans column-major (row index fastest) and keeps the first minimum
            struct Best { double min; int row, col; };
            std::vector<Best> best(nranges, Best{INFINITY, 0, 0});
            auto scan_range = [&](size_t r) {
                int c0, c1; range(r, c0, c1);
                Best bq{INFINITY, 0, 0};
                const double f = 0.5 / (dim - 2.0);
                for (int col = c0; col < c1; ++col) {
                    const double *colp = &tr[(size_t)act[(size_t)col] * ld];   // column col of the distances
                    const double sc = sums[(size_t)col];
                    for (int row = 0; row < dim; ++row) {
                        if (row == col) continue;
                        const double q = 0.5 * colp[(size_t)act[(size_t)row]] - f * (sc + sums[(size_t)row]);
                        if (q < bq.min) { bq.min = q; bq.row = row; bq.col = col; }
                    }
                }
                best[r] = bq;
            };
            if (threads) parallel_for(nranges, scan_range); else scan_range(0);
            double min = INFINITY;
            for (size_t r = 0; r < nranges; ++r) if (best[r].min < min) { min = best[r].min; index2 = best[r].row; index1 = best[r].col; }
            if (index2 < index1) std::swap(index1, index2);
        }
        double dist1 = (D(index1, index2) + (sums[index1] - sums[index2]) / (dim - 2.0)) / 2.0;
        dist1 = std::min(std::max(dist1, MIN_DIST), D(index1, index2));
        double dist2 = std::max(D(index2, index1) - dist1, MIN_DIST);
        double vsum = 0;
        for (int i = 0; i < dim; ++i) vsum += V(index2, i) - V(index1, i);
        double lambda = .5 + vsum / (2 * (dim - 2) * V(index1, index2));
        if (std::isnan(lambda)) lambda = .5;
        else lambda = std::min(std::max(0.0, lambda), 1.0);

        // reduce(index2) + the joined cluster in row / column index1 (TreeNJ.cpp:230-262)
        const double v12 = V(index1, index2);
        for (int i = 0; i < dim; ++i) {
            if (i == index2) continue;
            double nd = lambda * (D(index1, i) - dist1) + (1.0 - lambda) * (D(index2, i) - dist2);
            double nv = lambda * V(index1, i) + (1.0 - lambda) * V(index2, i) - lambda * (1.0 - lambda) * v12;
            if (i == index1) { nd = 0; nv = 0; }
            D(index1, i) = D(i, index1) = T(index1, i) = T(i, index1) = nd;
            V(index1, i) = V(i, index1) = nv;
        }
        act.erase(act.begin() + index2);
        fresh = index1;   // (index1 < index2: its reduced index stays)
        joins.push_back(pgm_bionj_join{(uint32_t)index1, (uint32_t)index2, dist1, dist2});
    }
    const int left = std::min(n0, 3);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) final_d[3 * r + c] = r < left && c < left ? D(r, c) : 0.0;
}

// The tree of a join record (TreeNJ.cpp:196-228 per join, :264-281 for the two or three clusters left)
PhyTree *bionj_tree(std::vector<std::string> seqs_order, const std::vector<pgm_bionj_join> &joins, const double *final_d) {
    const double MIN_DIST = 1e-4;
    std::vector<PhyTree *> subtrees;
    for (const std::string &s : seqs_order) subtrees.push_back(new PhyTree(s));
    for (const pgm_bionj_join &j : joins) {
        const size_t index1 = j.index1, index2 = j.index2;
        if (index1 >= index2 || index2 >= seqs_order.size()) error("BioNJ: join record out of range");
        std::string name1 = seqs_order[index1], name2 = seqs_order[index2];
        seqs_order.erase(seqs_order.begin() + (std::ptrdiff_t)index2);
        seqs_order[index1] = name1 + "," + name2;
        PhyTree *tree = new PhyTree(seqs_order[index1]);
        tree->addChild(subtrees[index1], j.dist1, support(j.dist1));
        tree->addChild(subtrees[index2], j.dist2, support(j.dist2));
        subtrees.erase(subtrees.begin() + (std::ptrdiff_t)index2);
        subtrees[index1] = tree;
    }
    auto D = [&](int i, int j) { return final_d[3 * i + j]; };
    PhyTree *tree = new PhyTree("root");
    if (seqs_order.size() == 2) {
        double d = D(0, 1) / 2;
        tree->addChild(subtrees[0], d, support(d));
        tree->addChild(subtrees[1], d, support(d));
    } else {
        double d0 = (D(0, 1) + D(0, 2) - D(1, 2)) / 2.0;
        d0 = std::min(std::max(d0, MIN_DIST), std::min(D(1, 0), D(2, 0)));
        double d1 = std::max(D(1, 0) - d0, MIN_DIST);
        double d2 = std::max(D(2, 0) - d0, MIN_DIST);
        PhyTree *tree2 = new PhyTree("root2");
        tree2->addChild(subtrees[0], d0, support(d0));
        tree2->addChild(subtrees[1], d1, support(d1));
        tree->addChild(subtrees[2], d2 / 2, support(d2));
        tree->addChild(tree2, d2 / 2, support(d2));
    }
    return tree;
}

PhyTree *buildNJTree(std::vector<std::string> seqs_order, DistanceMatrix dist, const PhyTree *topo) {
    std::vector<pgm_bionj_join> joins;
    double final_d[9];
    std::vector<pgm_bionj_pair> plan;
    if (topo) plan = build_topo_plan(seqs_order, topo);
    bionj_joins_host(std::move(dist), joins, final_d, topo ? &plan : nullptr);
    return bionj_tree(std::move(seqs_order), joins, final_d);
}

// ---- distances induced by an alignment (DistanceFactoryPrealigned.h:34-90) -----------------------------------------
// Pair counts over the columns where both rows have a residue (only residues with value() in 0..19, for every alphabet:
// the reference's literal 20), one gap per opening of a run in which exactly one of the two rows has a residue.
// a row of an alignment as the pair-count kernels read it: value() per residue, -1 for a gap, -2 for a residue without a value (and
// for the DNA unknown, value 4: the kernel counts every value below 20)
static void prealigned_row(const Alphabet &alphabet, const sequence_t &row, int8_t *out) {
    const bool dna = alphabet.kind == ALPHA_DNA;
    for (size_t k = 0; k < row.size(); ++k) {
        const int8_t c = row[k];
        const int v = alphabet.isGap(c) ? -1 : alphabet.value(c);
        out[k] = (int8_t)(alphabet.isGap(c) ? -1 : (v < 0 || (dna && v >= alphabet.DIM) ? -2 : v));
    }
}

// the same scan on the host (PGM_HOST_COUNTS, or a backend without the kernel): c is the pair's zeroed D x D count matrix; returns
// the gap openings
static uint32_t prealigned_count_pair(const Alphabet &alphabet, const sequence_t &s1, const sequence_t &s2, int32_t *c) {
    const size_t D = (size_t)alphabet.DIM;
    const int cmax = alphabet.kind == ALPHA_DNA ? (int)D : 20;   // (the DNA unknown is not counted: see the device rows above)
    uint32_t g = 0;
    bool open1 = false, open2 = false;
    for (size_t k = 0; k < s1.size(); ++k) {
        const bool g1 = alphabet.isGap(s1[k]), g2 = alphabet.isGap(s2[k]);
        if (!g1 && !g2) {
            const int c1 = alphabet.value(s1[k]), c2 = alphabet.value(s2[k]);
            if (c1 >= 0 && c1 < cmax && c2 >= 0 && c2 < cmax) ++c[(size_t)c1 + D * (size_t)c2];
            open1 = false; open2 = false;
        } else if (g1 && g2) {
            // skip
        } else if (!g1 && !open1) {
            ++g; open1 = true; open2 = false;
        } else if (!g2 && !open2) {
            ++g; open1 = false; open2 = true;
        }
    }
    return g;
}

// K = 2 for amino acids and codons, 6 for DNA (DistanceFactory.cpp:9-60): ncols = D^K = 400, 3721, 4096
static uint32_t angle_ncols(const Alphabet &a) {
    const uint32_t D = (uint32_t)a.DIM, K = a.kind == ALPHA_DNA ? 6u : 2u;
    uint32_t ncols = 1;
    for (uint32_t k = 0; k < K; ++k) ncols *= D;
    return ncols;
}
// DistanceFactoryAngle.h:63-94: the index of the last K values, none of them invalid (counts: one zeroed row of ncols)
static void angle_count_row(const Alphabet &a, const sequence_t &seq, uint32_t ncols, int32_t *counts) {
    const uint32_t D = (uint32_t)a.DIM, K = a.kind == ALPHA_DNA ? 6u : 2u;
    uint32_t index = 0, run = 0;   // (run: valid values at the end of the window so far)
    for (size_t j = 0; j < seq.size(); ++j) {
        const int v = a.value(seq[j]);
        if (v < 0 || v >= (int)D) { run = 0; index = 0; continue; }
        index = (index * D + (uint32_t)v) % ncols;
        if (++run >= K) counts[index] += 1;
    }
}
// from the cosine matrix as kmer_cosine wrote it to the distances and variances (DistanceFactoryAngle.h:100-113); `spread`: the rows
// on the host threads
static void angle_finish(DistanceMatrix &distances, const std::vector<double> &seq_len, bool spread) {
    const uint32_t n = (uint32_t)distances.dim;
    // kmer_cosine writes element (i, j) at i + n j (the reference's column-major matrix); DistanceMatrix::D(i, j) reads i n + j.  The
    // matrix is NOT symmetric in its last bits — ((c_i / |c_i|) . c_j) / |c_j| is rounded differently from the (j, i) element — and
    // BioNJ reads it by rows, by columns and at (index1, index2) / (index2, index1): the orientation has to be the reference's.
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) std::swap(distances.distances[(size_t)i * n + j], distances.distances[(size_t)j * n + i]);
    const bool ml = cmdlineopts.mldist_flag || cmdlineopts.mldist_gap_flag;
    // log and exp of the reference binary are those of the glibc it is linked with statically (2.17: IBM's correctly rounded ones);
    // today's libm is within 0.52 ulp, which moved the exact final tie of 3 trees in 60.  Correctly rounded here: the long double
    // function when its result is not within 2^-9 ulp of a rounding boundary, binary128 (libquadmath) otherwise.
    auto correctly_rounded = [](long double y, __float128 (*exact)(__float128), double x) {
        const double lo = (double)(y - fabsl(y) * 0x1p-62L), hi = (double)(y + fabsl(y) * 0x1p-62L);
        return lo == hi ? lo : (double)exact((__float128)x);
    };
    auto cr_log = [&](double x) { return correctly_rounded(logl((long double)x), logq, x); };
    auto cr_exp = [&](double x) { return correctly_rounded(expl((long double)x), expq, x); };
    auto row = [&](size_t r) {   // :101-105, row by row
        for (uint32_t c = 0; c < n; ++c) {
            double &d = distances.distances[r * n + c];
            d = -1.0 * cr_log((d * d + 0.4) / 1.4);
            if (!ml) {
                const double e = cr_exp(d);
                d = -0.5 * (5.0 * e - std::sqrt(45.0 * (e * e) - 20.0 * e)) * (1.0 / e);
            }
        }
    };
    if (spread) parallel_for((size_t)n, row);
    else for (size_t r = 0; r < n; ++r) row(r);
    for (uint32_t j = 0; j < n; ++j)   // :107-113: variances = distances / ((len_i + len_j) / 2), at least 1e-5
        for (uint32_t i = 0; i < n; ++i) {
            double v = 1.0 / ((seq_len[j] + seq_len[i]) / 2);
            v *= distances.D((int)i, (int)j);
            distances.V((int)i, (int)j) = std::max(v, 1e-5);
        }
}

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

double support(double d) {   // LeastSquares.cpp:16-23
    double s = 1.0 - std::exp(-std::log(2.0) * d / cmdlineopts.edge_halflife);
    s = std::min(1.0, std::max(0.0, s));
    if (std::isnan(s)) s = 0.0;
    return s;
}

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
            if (!quartetAround(e, nodes, edges)) { e->support = support(e->length); continue; }
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
        else g.edges[i].support = support(g.edges[i].length);
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


// ==== the guide tree: TreeNJ for one family, TreeNJ_multi for the families of a --batch chunk ===========================
// The defaults of the two multi-family entries: the per-family entries, one family after the other (a backend without segmented
// kernels of its own: the CPU oracle).
void Backend::kmer_cosine_multi(uint32_t nfam, const uint32_t *nseq, uint32_t ncols, const int32_t *counts, double *cosine, int worker) {
    size_t row0 = 0, out0 = 0;
    for (uint32_t f = 0; f < nfam; ++f) {
        kmer_cosine(nseq[f], ncols, counts + row0 * ncols, cosine + out0, worker);
        row0 += nseq[f];
        out0 += (size_t)nseq[f] * nseq[f];
    }
}

bool Backend::prealigned_counts_multi(uint32_t dim, uint32_t nfam, const uint32_t *nrows, const uint32_t *ncols, const int8_t *rows, uint32_t npairs,
                                      const uint32_t *fam, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) {
    std::vector<size_t> base(nfam + 1, 0);
    for (uint32_t f = 0; f < nfam; ++f) base[f + 1] = base[f] + (size_t)nrows[f] * ncols[f];
    std::vector<std::vector<uint32_t>> of_family(nfam);
    for (uint32_t p = 0; p < npairs; ++p) of_family[fam[p]].push_back(p);
    const size_t dd = (size_t)dim * dim;
    for (uint32_t f = 0; f < nfam; ++f) {
        const std::vector<uint32_t> &mine = of_family[f];
        if (mine.empty()) continue;
        const uint32_t m = (uint32_t)mine.size();
        std::vector<uint32_t> qi(m), qj(m), g(m, 0);
        std::vector<int32_t> c((size_t)m * dd, 0);
        for (uint32_t k = 0; k < m; ++k) { qi[k] = pi[mine[k]]; qj[k] = pj[mine[k]]; }
        if (!prealigned_counts_batch(dim, nrows[f], ncols[f], rows + base[f], m, qi.data(), qj.data(), c.data(), g.data(), worker)) return false;
        for (uint32_t k = 0; k < m; ++k) {
            std::copy(c.begin() + (std::ptrdiff_t)(k * dd), c.begin() + (std::ptrdiff_t)((k + 1) * dd), counts + (size_t)mine[k] * dd);
            gaps[mine[k]] = g[k];
        }
    }
    return true;
}

namespace {
// the pairs [p0, p0 + np) of a call's shared pair arrays are those of one family
struct PairBlock {
    const ModelFactory *model_factory;
    size_t p0;
    uint32_t np;
};

// The families of one call.  Their sequences stand one after the other in `seq` (family f: first[f] .. first[f + 1], in std::map key
// order like TreeNJ.h:34-39), their pairs i < j one after the other in pfam / pi / pj (family f: blocks[f]; pi, pj count within the
// family; df[f] estimates them into dist[f]).  One family is the solo run: first[0] = p0 = 0.
struct Families {
    uint32_t nfam = 0;
    std::vector<uint32_t> nseq, first;
    std::vector<const sequence_t *> seq;
    std::vector<std::vector<std::string>> order;
    std::vector<DistanceFactoryML> df;
    std::vector<DistanceMatrix> dist;
    std::vector<uint32_t> pfam, pi, pj;
    std::vector<PairBlock> blocks;
    const sequence_t &row(uint32_t f, uint32_t i) const { return *seq[first[f] + i]; }
    uint32_t np() const { return (uint32_t)pi.size(); }

    // the pairs i < j of every family, in row-major order or (the all-pairs farm) the longest pairs of a family first
    void all_pairs(bool longest_first) {
        for (uint32_t f = 0; f < nfam; ++f) {
            std::vector<std::pair<uint32_t, uint32_t>> pr;
            for (uint32_t i = 0; i < nseq[f]; ++i)
                for (uint32_t j = i + 1; j < nseq[f]; ++j) pr.push_back({i, j});
            if (longest_first) {
                auto cost = [&](const std::pair<uint32_t, uint32_t> &p) { return (uint64_t)row(f, p.first).size() * row(f, p.second).size(); };
                std::stable_sort(pr.begin(), pr.end(), [&](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return cost(x) > cost(y); });
            }
            blocks[f].p0 = pi.size();
            blocks[f].np = (uint32_t)pr.size();
            for (const auto &p : pr) { pfam.push_back(f); pi.push_back(p.first); pj.push_back(p.second); }
        }
    }
    void set(uint32_t p, double d, double v) {   // the estimate of pair p into its family's symmetric matrices
        DistanceMatrix &dm = dist[pfam[p]];
        dm.D(pi[p], pj[p]) = dm.D(pj[p], pi[p]) = d;
        dm.V(pi[p], pj[p]) = dm.V(pj[p], pi[p]) = v;
    }
};

// The model as pgm_mldist_batch takes it: in eigen form when it has one of at most 20 states, else in general form (Q alone: the
// 61-state ECM model, a generator that is not reversible)
pgm_mldist_model mldist_model(const Alphabet &a, const ModelFactory &mf, bool eigen_form) {
    double DIST_MAX, VAR_MAX, VAR_MIN;
    consts(a, DIST_MAX, VAR_MAX, VAR_MIN);
    pgm_mldist_model m;
    m.dim = (uint32_t)a.DIM; m.Q = mf.Qmat().data();
    m.V = eigen_form ? mf.eigV().data() : nullptr; m.Vi = eigen_form ? mf.eigVi().data() : nullptr;
    m.sigma = eigen_form ? mf.eigSigma().data() : nullptr;
    m.dist_max = DIST_MAX; m.var_max = VAR_MAX; m.var_min = VAR_MIN; m.cutoff_dist = cmdlineopts.cutoff_dist;
    m.min_dist = cmdlineopts.min_dist; m.max_dist = cmdlineopts.max_dist; m.indel_rate = cmdlineopts.indel_rate;
    m.mldist = cmdlineopts.mldist_flag ? 1 : 0; m.mldist_gap = cmdlineopts.mldist_gap_flag ? 1 : 0;
    return m;
}

// computeDistance of every pair from its count matrix.  On the device (PGM_DEVICE_MLDIST): one pgm_mldist_batch call over the pairs
// of all families that share a model — every family without -F, one call per family with it —, in the form that model takes (eigen
// form: one wavefront per pair, general form: one workgroup per pair, if the backend's kernel takes that); the arithmetic is
// computeDistance's except for the device library's exp / log (last-bit differences: see csrc/pgm_dist_kernels.h) and, for a model
// of more than 20 states that has an eigen form, P(d) = exp(Q d) by expm instead of that form.  Else on the host: Newton on d per
// pair, each step a P(d), independent per pair, so the pairs are dealt to the host threads; every pair's arithmetic is the
// single-threaded one, the matrix entries written are disjoint.
void estimate_distances(const Alphabet &a, Families &F, const int32_t *counts, const uint32_t *gaps, const double *seqlen) {
    const uint32_t D = (uint32_t)a.DIM;
    const size_t dd = (size_t)D * D;
    const std::vector<PairBlock> &blocks = F.blocks;
    Backend &be = default_backend();
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<char> on_device(blocks.size(), 0);
    if (host_switches().device_mldist)
        for (size_t b0 = 0; b0 < blocks.size();) {
            const size_t b1 = cmdlineopts.aafreqs_flag ? b0 + 1 : blocks.size();   // (the blocks are contiguous in the pair arrays)
            const ModelFactory &mf = *blocks[b0].model_factory;
            const bool eigen_form = mf.has_eigen() && D <= 20;
            const size_t p0 = blocks[b0].p0, p1 = blocks[b1 - 1].p0 + blocks[b1 - 1].np;
            bool ok = eigen_form || (be.mldist_general() && D <= 64);
            std::vector<double> dist(p1 - p0), var(p1 - p0);
            if (ok && p1 > p0) {
                const pgm_mldist_model m = mldist_model(a, mf, eigen_form);
                ++be.calls_dist;
                ok = be.mldist_batch(m, (uint32_t)(p1 - p0), counts + p0 * dd, gaps + p0, seqlen + p0, dist.data(), var.data());
            }
            for (size_t b = b0; b < b1 && ok; ++b) on_device[b] = 1;
            for (size_t p = p0; p < p1 && ok; ++p) F.set((uint32_t)p, dist[p - p0], var[p - p0]);
            b0 = b1;
        }
    std::vector<uint32_t> work;   // the pairs left to the host
    for (size_t b = 0; b < blocks.size(); ++b)
        for (uint32_t k = 0; k < blocks[b].np && !on_device[b]; ++k) work.push_back((uint32_t)blocks[b].p0 + k);
    const size_t grain = 16;   // pairs per index handed out
    parallel_for((work.size() + grain - 1) / grain, [&](size_t g) {
        std::vector<int32_t> c(dd);
        for (size_t q = g * grain; q < std::min(work.size(), (g + 1) * grain); ++q) {
            const size_t p = work[q];
            std::copy(counts + p * dd, counts + (p + 1) * dd, c.begin());
            const distvar_t dv = F.df[F.pfam[p]].computeDistance(c, gaps[p], seqlen[p]);
            F.set((uint32_t)p, dv.dist, dv.var);
        }
    });
    be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
}

// fn(w) for every worker w < nw, one host thread per device context (worker 0 on this thread).  An exception does not leave its
// thread (that would end the process): the first one is thrown here once all have joined.
void on_workers(int nw, const std::function<void(int)> &fn) {
    std::vector<std::string> errs((size_t)nw);
    auto run = [&](int w) { try { fn(w); } catch (std::exception &e) { errs[(size_t)w] = e.what(); } };
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(run, w);
    run(0);
    for (auto &t : th) t.join();
    for (const std::string &e : errs) if (!e.empty()) throw pgm_exception(e);
}

// symbols of the all-pairs alignment: value(), negative -> 20 for amino acids and codons (the reference's quirk,
// DistanceFactoryAlign.h:72,79); DNA has no negative values (sequenceFromString refuses other characters) and its unknown is DIM, the
// X row of its scoring matrix
void nw_symbols(const Alphabet &a, const std::vector<const sequence_t *> &seq, std::vector<int8_t> &syms, std::vector<uint32_t> &offs) {
    const int unknown_sym = a.kind == ALPHA_DNA ? a.DIM : 20;
    offs.assign(1, 0);
    for (const sequence_t *s : seq) {
        for (int8_t c : *s) {
            const int v = a.value(c);
            syms.push_back((int8_t)(v < 0 ? unknown_sym : v));
        }
        offs.push_back((uint32_t)syms.size());
    }
}

// The reference's i < j double loop (DistanceFactoryAlign.h:35-53) is a farm of independent alignPair jobs.  Here: the pairs (gi, gj:
// by their sequences' places among the nseq of the call) cut into tiles, and one host thread per device context pulling tile numbers
// from an atomic counter (no collective, no static partition: a slower device simply takes fewer tiles).  Every tile is one
// pgm_nw_pairs_submit call on the worker's own context; the outputs of a pair land at the pair's position, whoever computed it, so
// the result does not depend on the number of workers.
void nw_farm(const DistanceFactoryAlign &dfa, uint32_t D, uint32_t nseq, const std::vector<int8_t> &syms, const std::vector<uint32_t> &offs,
             const std::vector<uint32_t> &gi, const std::vector<uint32_t> &gj, bool reduced, int32_t *counts, uint32_t *gaps) {
    Backend &be = default_backend();
    const uint32_t np = (uint32_t)gi.size();
    const size_t per = reduced ? 2 : (size_t)D * D;
    const int nw = std::max(1, be.workers());
    // Tile size.  A call costs ~0.3 ms beside its kernel (staging of the inputs, launch, the last D2H: bench.py all_pairs_nw
    // rank0_fixed_ms_per_call) and a worker hides that of tile k under the kernel of tile k+1 (two tiles in flight), so what
    // matters is (a) that a tile fills a device — its persistent grid holds 7168 pairs at once; fewer pairs leave CUs idle —
    // and (b) that the last tiles of the ticket queue are small against a worker's share.  Three tiles per worker, at least
    // 256 pairs; the pairs are sorted by cost, so the last tiles are also the cheapest.  PGM_NW_TILE overrides.
    uint32_t tile = std::max<uint32_t>(256u, (np + 3u * (uint32_t)nw - 1u) / (3u * (uint32_t)nw));
    if (const char *e = getenv("PGM_NW_TILE")) tile = (uint32_t)std::max(1, atoi(e));
    const uint32_t ntiles = np ? (np + tile - 1) / tile : 0;
    std::atomic<uint32_t> next_tile(0);
    be.farm_workers = nw; be.farm_tiles = (int)ntiles;
    on_workers(nw, [&](int w) {
        int pending = -1;
        for (;;) {
            const uint32_t t = next_tile.fetch_add(1);
            if (t >= ntiles) break;
            const uint32_t p0 = t * tile, cnt = std::min(tile, np - p0);
            ++be.calls_dist;
            const int ticket = be.nw_pairs_submit(D, dfa.scoring_matrix().data(), dfa.gap_open, dfa.gap_extend, nseq, syms.data(), offs.data(), cnt,
                                                  gi.data() + p0, gj.data() + p0, reduced ? 1u : 0u, counts + (size_t)p0 * per, gaps + p0, w);
            if (pending >= 0) be.nw_pairs_wait(pending, w);
            pending = ticket;
        }
        if (pending >= 0) be.nw_pairs_wait(pending, w);
    });
}

// -a (DistanceFactoryAlign.h:29-56): one farm of alignPair tiles over the sequences of all families, within-family pairs only
void nw_distances(const Alphabet &a, Families &F) {
    const uint32_t D = (uint32_t)a.DIM;
    Backend &be = default_backend();
    DistanceFactoryAlign dfa(a, F.blocks[0].model_factory);   // (the scoring matrix and the gap costs: the run's)
    std::vector<int8_t> syms;
    std::vector<uint32_t> offs;
    nw_symbols(a, F.seq, syms, offs);
    F.all_pairs(true);
    const uint32_t np = F.np();
    std::vector<uint32_t> gi(np), gj(np);
    for (uint32_t p = 0; p < np; ++p) { gi[p] = F.first[F.pfam[p]] + F.pi[p]; gj[p] = F.first[F.pfam[p]] + F.pj[p]; }
    auto len = [&](uint32_t s) { return offs[s + 1] - offs[s]; };
    // Without --mldist / --mldist_gap the distance of a pair reads (ident, total) of its count matrix and nothing else
    // (DistanceFactoryML.h:143-146, 175-178): the device reduces them and 8 B per pair come back instead of 4 D^2.
    const bool reduced = !(cmdlineopts.mldist_flag || cmdlineopts.mldist_gap_flag);
    const size_t per = reduced ? 2 : (size_t)D * D;
    // result buffers in pinned memory (the D2H copies write them directly), not zero-filled: every pair's slice is written by its tile
    int32_t *counts = (int32_t *)be.host_alloc(std::max<size_t>(sizeof(int32_t) * (size_t)np * per, 16));
    uint32_t *gaps = (uint32_t *)be.host_alloc(std::max<size_t>(4 * (size_t)np, 16));
    try {
        for (uint32_t p = 0; p < np; ++p) be.cells_nw += (uint64_t)len(gi[p]) * len(gj[p]);
        const auto t0 = std::chrono::steady_clock::now();
        nw_farm(dfa, D, (uint32_t)F.seq.size(), syms, offs, gi, gj, reduced, counts, gaps);
        be.seconds_nw += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<double> seqlen(np);
        for (uint32_t p = 0; p < np; ++p) seqlen[p] = ((double)len(gi[p]) + (double)len(gj[p])) / 2.0;
        if (reduced) {
            for (uint32_t p = 0; p < np; ++p) {
                const distvar_t dv = F.df[F.pfam[p]].computeDistance((double)counts[2 * (size_t)p], (double)counts[2 * (size_t)p + 1], nullptr, gaps[p], seqlen[p]);
                F.set(p, dv.dist, dv.var);
            }
        } else {
            estimate_distances(a, F, counts, gaps, seqlen.data());
        }
    } catch (...) {
        be.host_free(counts);
        be.host_free(gaps);
        throw;
    }
    be.host_free(counts);
    be.host_free(gaps);
}

// Distances induced by the families' alignments: pair counts on the device (integer counts, bit-exact: on by default, unlike the ML
// estimates that follow), on the host threads with PGM_HOST_COUNTS or a backend without the kernel, then the estimates.
// per_family_calls: see tree_nj.
void prealigned_distances(const Alphabet &a, Families &F, bool per_family_calls) {
    const uint32_t D = (uint32_t)a.DIM, nfam = F.nfam;
    const size_t dd = (size_t)D * D;
    Backend &be = default_backend();
    F.all_pairs(false);
    const uint32_t np = F.np();
    std::vector<uint32_t> ncols(nfam);
    for (uint32_t f = 0; f < nfam; ++f) ncols[f] = (uint32_t)F.row(f, 0).size();
    std::vector<int32_t> counts((size_t)np * dd, 0);
    std::vector<uint32_t> gaps(np, 0);
    bool done = false;
    if (!host_switches().host_counts) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<size_t> base(nfam + 1, 0);   // every family's nseq x ncols matrix, back to back
        for (uint32_t f = 0; f < nfam; ++f) base[f + 1] = base[f] + (size_t)F.nseq[f] * ncols[f];
        std::vector<int8_t> mat(base[nfam]);
        parallel_for(nfam, [&](size_t f) {
            for (uint32_t i = 0; i < F.nseq[f]; ++i) prealigned_row(a, F.row((uint32_t)f, i), mat.data() + base[f] + (size_t)i * ncols[f]);
        });
        // The entry points take 20 to 64 states: DNA rows (values 0..3, -2) are counted as 20-state rows and the 4 x 4 corner of each
        // 20 x 20 matrix is kept
        const uint32_t Dk = std::max<uint32_t>(D, 20u);
        std::vector<int32_t> wide(Dk != D ? (size_t)np * Dk * Dk : 0, 0);
        int32_t *const cdst = Dk != D ? wide.data() : counts.data();
        done = true;
        if (!per_family_calls) {
            ++be.calls_dist;
            done = be.prealigned_counts_multi(Dk, nfam, F.nseq.data(), ncols.data(), mat.data(), np, F.pfam.data(), F.pi.data(), F.pj.data(), cdst, gaps.data());
        } else
            for (uint32_t f = 0; f < nfam; ++f) {
                // every pair costs the same (one scan of the columns): contiguous ranges of the family's pairs, one per device context
                const size_t q0 = F.blocks[f].p0;
                const uint32_t nq = F.blocks[f].np;
                const int nw = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, be.workers()), nq));
                std::vector<char> ok((size_t)nw, 0);
                on_workers(nw, [&](int w) {
                    const uint32_t p0 = (uint32_t)((uint64_t)nq * (uint32_t)w / (uint32_t)nw), p1 = (uint32_t)((uint64_t)nq * ((uint32_t)w + 1u) / (uint32_t)nw);
                    if (p1 != p0) ++be.calls_dist;
                    ok[(size_t)w] = (p1 == p0 || be.prealigned_counts_batch(Dk, F.nseq[f], ncols[f], mat.data() + base[f], p1 - p0, F.pi.data() + q0 + p0,
                                                                           F.pj.data() + q0 + p0, cdst + (q0 + p0) * Dk * Dk, gaps.data() + q0 + p0, w)) ? 1 : 0;
                });
                for (char c : ok) done = done && c;
            }
        if (done && Dk != D)
            for (size_t p = 0; p < np; ++p)
                for (uint32_t b = 0; b < D; ++b)
                    for (uint32_t c = 0; c < D; ++c) counts[p * dd + c + (size_t)D * b] = wide[p * Dk * Dk + c + (size_t)Dk * b];
        be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!done) {
        const auto t1 = std::chrono::steady_clock::now();
        const size_t grain = 16;   // pairs per index handed out
        parallel_for(((size_t)np + grain - 1) / grain, [&](size_t g) {
            for (size_t p = g * grain; p < std::min<size_t>(np, (g + 1) * grain); ++p) {
                std::fill(counts.begin() + (std::ptrdiff_t)(p * dd), counts.begin() + (std::ptrdiff_t)((p + 1) * dd), 0);   // (a device call that failed may have written)
                gaps[p] = prealigned_count_pair(a, F.row(F.pfam[p], F.pi[p]), F.row(F.pfam[p], F.pj[p]), counts.data() + p * dd);
            }
        });
        be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    }
    std::vector<double> seqlen(np);
    for (size_t p = 0; p < np; ++p) seqlen[p] = ((double)ncols[F.pfam[p]] + (double)ncols[F.pfam[p]]) / 2.0;
    const auto tq0 = std::chrono::steady_clock::now();
    estimate_distances(a, F, counts.data(), gaps.data(), seqlen.data());
    if (host_switches().profile && nfam == 1)
        fprintf(stderr, "  prealigned distances: pair counts %s, estimates %.1f ms\n", done ? "on the device" : "on the host",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq0).count());
}

// DistanceFactory::getDefault (DistanceFactory.cpp:9-20), DistanceFactoryAngle<ALPHABET, K> (DistanceFactoryAngle.h:55-131): the
// default initial distances (no -a), the cosine of the k-mer count vectors turned into a distance.  The count rows of all families
// back to back; per_family_calls: see tree_nj.
void angle_distances(const Alphabet &a, Families &F, bool per_family_calls) {
    const uint32_t nfam = F.nfam, ncols = angle_ncols(a);
    Backend &be = default_backend();
    std::vector<size_t> out0(nfam + 1, 0);
    for (uint32_t f = 0; f < nfam; ++f) out0[f + 1] = out0[f] + (size_t)F.nseq[f] * F.nseq[f];
    std::vector<int32_t> counts(F.seq.size() * ncols, 0);
    std::vector<double> cosine(out0[nfam], 0.0);
    parallel_for(F.seq.size(), [&](size_t s) { angle_count_row(a, *F.seq[s], ncols, counts.data() + s * ncols); });
    const auto t0 = std::chrono::steady_clock::now();
    if (!per_family_calls) {
        ++be.calls_dist;
        be.kmer_cosine_multi(nfam, F.nseq.data(), ncols, counts.data(), cosine.data());
    } else
        for (uint32_t f = 0; f < nfam; ++f) {
            ++be.calls_dist;
            be.kmer_cosine(F.nseq[f], ncols, counts.data() + (size_t)F.first[f] * ncols, cosine.data() + out0[f]);   // :100
        }
    be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // one family: its rows on the host threads; several: the families
    parallel_for(nfam, [&](size_t f) {
        std::copy(cosine.begin() + (std::ptrdiff_t)out0[f], cosine.begin() + (std::ptrdiff_t)out0[f + 1], F.dist[f].distances.begin());
        std::vector<double> seq_len(F.nseq[f]);
        for (uint32_t i = 0; i < F.nseq[f]; ++i) seq_len[i] = (double)F.row((uint32_t)f, i).size();
        angle_finish(F.dist[f], seq_len, nfam == 1);
    });
}

// BioNJ's joins of the families whose matrices are `dist` (nseq[f] taxa each; plan_of(f): the pairs a fixed topology prescribes, or
// nullptr): the join record and final_d of every family, and the message of a family whose joins failed.  The route is described
// inside; tree_nj and the bootstrap replicates share it.
void bionj_joins_families(std::vector<DistanceMatrix> &dist, const std::vector<uint32_t> &nseq,
                          const std::function<const std::vector<pgm_bionj_pair> *(uint32_t)> &plan_of, std::vector<std::vector<pgm_bionj_join>> &joins,
                          std::vector<double> &final_d, std::vector<std::string> &join_error) {
    const auto tq1 = std::chrono::steady_clock::now();
    Backend &be_bionj = default_backend();
    const uint32_t nfam = (uint32_t)dist.size();
    // BioNJ's joins: one bionj_multi call over the families of 4 taxa and more on worker 0 (PGM_DEVICE_BIONJ, or by default when
    // the largest family has kBionjDeviceMin taxa and every entry is finite: the device entry takes no NaN or infinity), or the
    // host loop per family (one family: on this thread, the loop's sections on the host threads; several: the families on the
    // host threads).  Either way the same join records, and so the same trees.
    // The families with a fixed topology are a call of their own, bionj_plan_multi, with PGM_DEVICE_BIONJ only: their host loop
    // is O(n) per join as well, so it is the default.
    joins.assign(nfam, std::vector<pgm_bionj_join>());
    final_d.assign((size_t)9 * nfam, 0.0);
    for (DistanceMatrix &d : dist)
        for (int i = 0; i < d.dim; ++i) { d.D(i, i) = 0; d.V(i, i) = 0; }
    std::vector<char> on_device(nfam, 0);
    for (int planned = 0; planned < 2; ++planned) {
        std::vector<uint32_t> dev;   // the families of the device call
        uint32_t nmax = 0;
        for (uint32_t f = 0; f < nfam; ++f)
            if ((plan_of(f) != nullptr) == (planned != 0) && nseq[f] >= 4 && nseq[f] <= PGM_BIONJ_MAX_N) { dev.push_back(f); nmax = std::max(nmax, nseq[f]); }
        const HostSwitches &sw = host_switches();
        if (!dev.empty() && !sw.host_bionj && (sw.device_bionj || (!planned && nmax >= kBionjDeviceMin))) {
            std::vector<char> finite(dev.size(), 1);
            parallel_for(dev.size(), [&](size_t k) {
                const DistanceMatrix &d = dist[dev[k]];
                bool ok = true;
                for (size_t e = 0; e < d.distances.size(); ++e) ok = ok && std::isfinite(d.distances[e]) && std::isfinite(d.variances[e]);
                finite[k] = ok ? 1 : 0;
            });
            bool all_finite = true;
            for (char c : finite) all_finite = all_finite && c;
            if (all_finite) {
                std::vector<uint32_t> ns(dev.size());
                std::vector<size_t> m0(dev.size() + 1, 0), j0(dev.size() + 1, 0);
                for (size_t k = 0; k < dev.size(); ++k) {
                    ns[k] = nseq[dev[k]];
                    m0[k + 1] = m0[k] + (size_t)ns[k] * ns[k];
                    j0[k + 1] = j0[k] + ns[k] - 3;
                }
                std::vector<double> Dcat, Vcat;   // (one family: its own matrices)
                if (dev.size() > 1) {
                    Dcat.resize(m0[dev.size()]); Vcat.resize(m0[dev.size()]);
                    parallel_for(dev.size(), [&](size_t k) {
                        const DistanceMatrix &d = dist[dev[k]];
                        std::copy(d.distances.begin(), d.distances.end(), Dcat.begin() + (std::ptrdiff_t)m0[k]);
                        std::copy(d.variances.begin(), d.variances.end(), Vcat.begin() + (std::ptrdiff_t)m0[k]);
                    });
                }
                const DistanceMatrix &d0 = dist[dev[0]];
                const double *Dp = dev.size() > 1 ? Dcat.data() : d0.distances.data(), *Vp = dev.size() > 1 ? Vcat.data() : d0.variances.data();
                std::vector<pgm_bionj_join> jcat(j0[dev.size()]);
                std::vector<double> fcat((size_t)9 * dev.size());
                bool ran;
                if (planned) {
                    std::vector<pgm_bionj_pair> pcat(j0[dev.size()]);   // (a plan has n - 1 pairs: the joins use the first n - 3)
                    for (size_t k = 0; k < dev.size(); ++k) std::copy(plan_of(dev[k])->begin(), plan_of(dev[k])->begin() + (std::ptrdiff_t)(ns[k] - 3), pcat.begin() + (std::ptrdiff_t)j0[k]);
                    ran = be_bionj.bionj_plan_multi((uint32_t)dev.size(), ns.data(), Dp, Vp, pcat.data(), jcat.data(), fcat.data(), 0);
                } else {
                    ran = be_bionj.bionj_multi((uint32_t)dev.size(), ns.data(), Dp, Vp, jcat.data(), fcat.data(), 0);
                }
                if (ran)
                    for (size_t k = 0; k < dev.size(); ++k) {
                        on_device[dev[k]] = 1;
                        joins[dev[k]].assign(jcat.begin() + (std::ptrdiff_t)j0[k], jcat.begin() + (std::ptrdiff_t)j0[k + 1]);
                        std::copy(fcat.begin() + (std::ptrdiff_t)(9 * k), fcat.begin() + (std::ptrdiff_t)(9 * k + 9), final_d.begin() + (std::ptrdiff_t)(9 * (size_t)dev[k]));
                    }
            }
        }
    }
    join_error.assign(nfam, std::string());
    parallel_for(nfam, [&](size_t f) {
        if (on_device[f]) return;
        try { bionj_joins_host(dist[f], joins[f], &final_d[9 * f], plan_of((uint32_t)f)); }
        catch (std::exception &e) { join_error[f] = e.what(); }
    });
    be_bionj.seconds_bionj += std::chrono::duration<double>(std::chrono::steady_clock::now() - tq1).count();
}

// TreeNJ.h:27-59 for a list of families: one of the three distance stages over the pairs of all of them, then BioNJ, the -W
// refinement (TreeNJ.h:52-54) and the rooting per family.  per_family_calls is all that tells the two entry points apart: the
// cosine matrix and the pair counts of an alignment through the per-family entries of the backend (TreeNJ: kmer_cosine, and
// prealigned_counts_batch over every device context), or through the entries that take all families in one call on worker 0
// (TreeNJ_multi).  Either way a family's matrices, and so its tree, are the same.
void tree_nj(const Alphabet &a, std::vector<TreeJob> &jobs, bool prealigned, bool per_family_calls) {
    const auto tq0 = std::chrono::steady_clock::now();
    std::vector<size_t> act;
    for (size_t j = 0; j < jobs.size(); ++j) {
        jobs[j].tree = nullptr;
        jobs[j].error.clear();
        if (jobs[j].seqs->size() < 2) { jobs[j].error = "cannot construct tree from < 2 sequences"; continue; }
        if (prealigned) {
            const size_t L = jobs[j].seqs->begin()->second.size();
            bool same = true;
            for (const auto &kv : *jobs[j].seqs) same = same && kv.second.size() == L;
            if (!same) { jobs[j].error = "prealigned distances: rows of different length"; continue; }
        }
        act.push_back(j);
    }
    // the plans of the families with a fixed topology (std::map key order is the order of the matrix: TreeNJ.h:34-39); a family
    // whose topology does not fit leaves with the message before any distance is estimated
    std::vector<std::vector<pgm_bionj_pair>> plans(jobs.size());
    {
        std::vector<size_t> fits;
        for (size_t j : act) {
            if (jobs[j].topo) {
                std::vector<std::string> order;
                for (const auto &kv : *jobs[j].seqs) order.push_back(kv.first);
                try { plans[j] = build_topo_plan(order, jobs[j].topo); }
                catch (std::exception &e) { jobs[j].error = e.what(); continue; }
            }
            fits.push_back(j);
        }
        act.swap(fits);
    }
    if (act.empty()) return;
    Families F;
    const uint32_t nfam = F.nfam = (uint32_t)act.size();
    F.nseq.resize(nfam); F.first.resize(nfam); F.order.resize(nfam); F.blocks.resize(nfam);
    for (uint32_t f = 0; f < nfam; ++f) {
        const TreeJob &job = jobs[act[f]];
        F.first[f] = (uint32_t)F.seq.size();
        for (const auto &kv : *job.seqs) { F.order[f].push_back(kv.first); F.seq.push_back(&kv.second); }
        F.nseq[f] = (uint32_t)F.order[f].size();
        F.df.emplace_back(a, job.model_factory);
        F.dist.emplace_back((int)F.nseq[f]);
        F.blocks[f] = PairBlock{job.model_factory, 0, 0};
    }
    if (prealigned) prealigned_distances(a, F, per_family_calls);
    else if (!cmdlineopts.nwdist_flag) angle_distances(a, F, per_family_calls);
    else nw_distances(a, F);
    for (const DistanceMatrix &d : F.dist) dump_distances(d);   // (--dump_dist: refused with --batch, so one matrix per call)
    const auto tq1 = std::chrono::steady_clock::now();
    std::vector<std::vector<pgm_bionj_join>> joins;
    std::vector<double> final_d;
    std::vector<std::string> join_error;
    auto plan_of = [&](uint32_t f) -> const std::vector<pgm_bionj_pair> * { return jobs[act[f]].topo ? &plans[act[f]] : nullptr; };
    bionj_joins_families(F.dist, F.nseq, plan_of, joins, final_d, join_error);
    for (uint32_t f = 0; f < nfam; ++f) dump_joins((int32_t)F.nseq[f], joins[f], &final_d[9 * (size_t)f]);   // (--dump_joins: refused with --batch)
    // the trees, -W and the rooting per family on the host threads (-W is refused with --batch: refineTree loads one tree's
    // matrices into the backend)
    parallel_for(nfam, [&](size_t f) {
        TreeJob &job = jobs[act[f]];
        try {
            if (!join_error[f].empty()) throw pgm_exception(join_error[f]);
            DistanceMatrix &d = F.dist[f];
            PhyTree *tree = bionj_tree(F.order[f], joins[f], &final_d[9 * f]);
            if (cmdlineopts.wlsrefine_flag) tree = refineTree(tree, F.order[f], d);
            job.tree = midpointRoot(tree);
        } catch (std::exception &e) { job.error = e.what(); }
    });
    if (host_switches().profile && prealigned && nfam == 1)
        fprintf(stderr, "  TreeNJ: distances %.1f ms, BioNJ + rooting %.1f ms\n", std::chrono::duration<double, std::milli>(tq1 - tq0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq1).count());
}
}  // namespace

PhyTree *TreeNJ(const Alphabet &a, const std::map<std::string, sequence_t> &seqs, const ModelFactory *mf, bool prealigned, const PhyTree *topo) {
    std::vector<TreeJob> job(1);
    job[0].seqs = &seqs;
    job[0].model_factory = mf;
    job[0].topo = topo;
    tree_nj(a, job, prealigned, true);
    if (!job[0].error.empty()) throw pgm_exception(job[0].error);
    return job[0].tree;
}

void TreeNJ_multi(const Alphabet &a, std::vector<TreeJob> &jobs, bool prealigned) { tree_nj(a, jobs, prealigned, false); }

// ==== --bootstrap: the trees of resampled columns of one alignment =====================================================
BootstrapStats bootstrap_stats;

uint64_t splitmix64(uint64_t &state) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bool Backend::prealigned_counts_resampled(uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t nrep, const uint32_t *cols,
                                          uint32_t npairs, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) {
    std::vector<int8_t> gathered((size_t)nrows * ncols);
    for (uint32_t r = 0; r < nrep; ++r) {
        const uint32_t *c = cols + (size_t)r * ncols;
        for (uint32_t i = 0; i < nrows; ++i)
            for (uint32_t k = 0; k < ncols; ++k) gathered[(size_t)i * ncols + k] = rows[(size_t)i * ncols + c[k]];
        if (!prealigned_counts_batch(dim, nrows, ncols, gathered.data(), npairs, pi, pj, counts + (size_t)r * npairs * dim * dim, gaps + (size_t)r * npairs, worker))
            return false;
    }
    return true;
}

std::vector<PhyTree *> bootstrap_trees(const Alphabet &a, const std::map<std::string, sequence_t> &rows, const ModelFactory *mf, uint32_t nrep, uint64_t seed) {
    const uint32_t n = (uint32_t)rows.size(), D = (uint32_t)a.DIM;
    if (n < 4) error("bootstrap: fewer than 4 sequences");
    const size_t L = rows.begin()->second.size();
    std::vector<std::string> order;   // (std::map key order: the order of the matrices, TreeNJ.h:34-39)
    std::vector<const sequence_t *> seq;
    for (const auto &kv : rows) {
        if (kv.second.size() != L) error("bootstrap: rows of different length");
        order.push_back(kv.first);
        seq.push_back(&kv.second);
    }
    if (L == 0 || L > 0xffffffffull) error("bootstrap: an alignment of %zu columns", L);
    const uint32_t ncols = (uint32_t)L;
    Backend &be = default_backend();
    std::vector<int8_t> mat((size_t)n * ncols);
    parallel_for(n, [&](size_t i) { prealigned_row(a, *seq[i], mat.data() + i * ncols); });
    std::vector<uint32_t> cols((size_t)nrep * ncols);
    uint64_t state = seed;
    for (size_t k = 0; k < cols.size(); ++k) cols[k] = (uint32_t)(splitmix64(state) % ncols);
    std::vector<uint32_t> pi, pj;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) { pi.push_back(i); pj.push_back(j); }
    const uint32_t np = (uint32_t)pi.size();
    // The entry points count 20 to 64 states (prealigned_distances): DNA keeps the 4 x 4 corner of each 20 x 20 matrix
    const uint32_t Dk = std::max<uint32_t>(D, 20u);
    const size_t dd = (size_t)D * D, ddk = (size_t)Dk * Dk;
    const uint32_t group = (uint32_t)std::max<size_t>(1, std::min<size_t>(nrep, kBootstrapCountBytes / (sizeof(int32_t) * ddk * np)));
    std::vector<PhyTree *> trees(nrep, nullptr);
    try {
        std::vector<int32_t> wide, counts;
        std::vector<uint32_t> gaps;
        std::vector<int8_t> gathered;
        for (uint32_t r0 = 0; r0 < nrep; r0 += group) {
            const uint32_t g = std::min(group, nrep - r0);
            const size_t gp = (size_t)g * np;
            const uint32_t *gcols = cols.data() + (size_t)r0 * ncols;
            counts.assign(gp * dd, 0);
            gaps.assign(gp, 0);
            bool done = false;
            if (!host_switches().host_counts) {
                const auto t0 = std::chrono::steady_clock::now();
                if (Dk != D) wide.assign(gp * ddk, 0);
                int32_t *const cdst = Dk != D ? wide.data() : counts.data();
                ++bootstrap_stats.counts_calls;
                ++be.calls_dist;
                done = be.prealigned_counts_resampled(Dk, n, ncols, mat.data(), g, gcols, np, pi.data(), pj.data(), cdst, gaps.data());
                if (done && Dk != D)
                    for (size_t p = 0; p < gp; ++p)
                        for (uint32_t b = 0; b < D; ++b)
                            for (uint32_t c = 0; c < D; ++c) counts[p * dd + c + (size_t)D * b] = wide[p * ddk + c + (size_t)Dk * b];
                be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            }
            if (!done) {   // (PGM_HOST_COUNTS, or a backend without the kernel: the host's scan of the gathered rows)
                const auto t1 = std::chrono::steady_clock::now();
                std::fill(counts.begin(), counts.end(), 0);
                for (uint32_t r = 0; r < g; ++r) {
                    std::vector<sequence_t> grow(n, sequence_t(ncols, 0));
                    parallel_for(n, [&](size_t i) { for (uint32_t k = 0; k < ncols; ++k) grow[i][k] = (*seq[i])[gcols[(size_t)r * ncols + k]]; });
                    parallel_for(np, [&](size_t p) { gaps[(size_t)r * np + p] = prealigned_count_pair(a, grow[pi[p]], grow[pj[p]], counts.data() + ((size_t)r * np + p) * dd); });
                }
                be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
            }
            // the replicates of the group as families of one call: the estimator and the joins of tree_nj
            Families F;
            F.nfam = g;
            F.nseq.assign(g, n);
            F.blocks.resize(g);
            for (uint32_t f = 0; f < g; ++f) {
                F.df.emplace_back(a, mf);
                F.dist.emplace_back((int)n);
                F.blocks[f] = PairBlock{mf, (size_t)f * np, np};
                for (uint32_t p = 0; p < np; ++p) { F.pfam.push_back(f); F.pi.push_back(pi[p]); F.pj.push_back(pj[p]); }
            }
            const std::vector<double> seqlen(gp, ((double)ncols + (double)ncols) / 2.0);
            estimate_distances(a, F, counts.data(), gaps.data(), seqlen.data());
            std::vector<std::vector<pgm_bionj_join>> joins;
            std::vector<double> final_d;
            std::vector<std::string> join_error;
            bionj_joins_families(F.dist, F.nseq, [](uint32_t) -> const std::vector<pgm_bionj_pair> * { return nullptr; }, joins, final_d, join_error);
            for (uint32_t f = 0; f < g; ++f) {
                if (!join_error[f].empty()) throw pgm_exception(join_error[f]);
                trees[r0 + f] = bionj_tree(order, joins[f], &final_d[9 * (size_t)f]);
            }
        }
    } catch (...) {
        for (PhyTree *t : trees) delete t;
        throw;
    }
    bootstrap_stats.replicates += (int)nrep;
    return trees;
}
}  // namespace pgm
