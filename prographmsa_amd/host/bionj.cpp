// bionj.cpp — the BioNJ guide tree and the plan of a fixed topology (reference src/TreeNJ.{h,cpp}).
// The joins of neighbour joining on the host threads (bionj_joins_host) or, from kBionjDeviceMin taxa on, behind pgm_bionj_multi
// (bionj_joins_families decides per call); with a fixed topology (--topology) the pairs come from a plan (build_topo_plan); the
// tree of a join record (bionj_tree).
#include "pgm_host.h"
#include <algorithm>
#include <chrono>
#include <cmath>

namespace pgm {
// ---- BioNJ (TreeNJ.cpp:22-29, 132-281; the plan of a fixed topology: TreeNJ.cpp:31-130) -------------
double edge_support(double d) {   // TreeNJ.cpp:22-29, LeastSquares.cpp:16-23
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
        tree->addChild(subtrees[index1], j.dist1, edge_support(j.dist1));
        tree->addChild(subtrees[index2], j.dist2, edge_support(j.dist2));
        subtrees.erase(subtrees.begin() + (std::ptrdiff_t)index2);
        subtrees[index1] = tree;
    }
    auto D = [&](int i, int j) { return final_d[3 * i + j]; };
    PhyTree *tree = new PhyTree("root");
    if (seqs_order.size() == 2) {
        double d = D(0, 1) / 2;
        tree->addChild(subtrees[0], d, edge_support(d));
        tree->addChild(subtrees[1], d, edge_support(d));
    } else {
        double d0 = (D(0, 1) + D(0, 2) - D(1, 2)) / 2.0;
        d0 = std::min(std::max(d0, MIN_DIST), std::min(D(1, 0), D(2, 0)));
        double d1 = std::max(D(1, 0) - d0, MIN_DIST);
        double d2 = std::max(D(2, 0) - d0, MIN_DIST);
        PhyTree *tree2 = new PhyTree("root2");
        tree2->addChild(subtrees[0], d0, edge_support(d0));
        tree2->addChild(subtrees[1], d1, edge_support(d1));
        tree->addChild(subtrees[2], d2 / 2, edge_support(d2));
        tree->addChild(tree2, d2 / 2, edge_support(d2));
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

// BioNJ's joins of the families whose matrices are `dist` (nseq[f] taxa each; plan_of(f): the pairs a fixed topology prescribes, or
// nullptr): the join record and final_d of every family, and the message of a family whose joins failed.  The route is described
// inside; tree_nj and the bootstrap replicates (distance.cpp) share it.
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
}  // namespace pgm
