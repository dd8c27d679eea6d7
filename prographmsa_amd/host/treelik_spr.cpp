// treelik_spr.cpp — subtree pruning and regrafting for `pgmsa --ml_tree --ml_search --ml_spr` (the walk and the
// checks are treelik_internal.h's): the host statement of pgm_tree_spr (Backend::tree_spr's default, what pgmsa_oracle runs), the
// lister of a tree's candidates within a radius, the move applied to a numbered tree, and the scan ml_topology_search runs where
// its interchanges stall, which is host code and the same for every backend.
#include "treelik_internal.h"

#include <chrono>
#include <numeric>

namespace pgm {

void tree_spr_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                   const double *w, const double *P, const double *Ph, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_y, double *site_l, int32_t *site_k,
                   double *post, double *rho, size_t block_bytes) {
    if (!w || !post || !Ph || !cand_v || !cand_y || !rho) error("tree likelihood: null argument");
    treelik_check_rates_host(ncat, w);
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, 0, site_l, site_k, nullptr, nullptr);
    std::vector<uint32_t> path;
    const std::string bad = pgm_treelik_check_spr(nnodes, parent, ch.off, ncand, cand_v, cand_y, path);
    if (!bad.empty()) error("%s", bad.c_str());
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves, root = nnodes - 1;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk, mat = (size_t)dim * dim, pstride = mat * nedges;
    // the candidates grouped by their prune node (the groups in the order of their first candidate, a group's in the given order):
    // a work item is a prune node and a column chunk
    std::vector<uint32_t> order(ncand), group_off;
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cand_v[a] < cand_v[b]; });
    for (uint32_t k = 0; k < ncand; ++k)
        if (k == 0 || cand_v[order[k]] != cand_v[order[k - 1]]) group_off.push_back(k);
    const size_t ngroups = group_off.size();
    group_off.push_back(ncand);
    // the partials and the outside vectors of a block of column chunks at a time, as tree_nni_host holds them
    const size_t vstride = (size_t)ninner * dim, per_chunk = 2 * 8 * vstride * ncat * kTreelikChunk;
    const size_t block_chunks = std::min(nchunks, std::max<size_t>(1, block_bytes / per_chunk));
    const size_t cstride = vstride * block_chunks * kTreelikChunk;
    std::vector<double> U(cstride * ncat), O(cstride * ncat);
    for (size_t chunk0 = 0; chunk0 < nchunks; chunk0 += block_chunks) {
        const size_t chunks_here = std::min(block_chunks, nchunks - chunk0), site0 = chunk0 * kTreelikChunk;

        parallel_for(chunks_here, [&](size_t rel) {
            const size_t chunk = chunk0 + rel;
            TreelikSiteWalk walk(ch, dim, nleaves, nnodes, ncols, rows, pi, false, true);
            std::vector<double> L(ncat);
            std::vector<int32_t> k(ncat);
            const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
            for (uint32_t s = s0; s < s1; ++s) {
                for (uint32_t c = 0; c < ncat; ++c) {
                    walk(s, P + pstride * c, L[c], k[c], nullptr, nullptr);
                    walk.posteriors(s, P + pstride * c, nullptr);
                    std::copy(walk.U.begin(), walk.U.end(), U.begin() + cstride * c + vstride * (s - site0));
                    std::copy(walk.O.begin(), walk.O.end(), O.begin() + cstride * c + vstride * (s - site0));
                }
                int32_t kmin = k[0];
                for (uint32_t c = 1; c < ncat; ++c) kmin = k[c] < kmin ? k[c] : kmin;
                double total = 0.0;
                for (uint32_t c = 0; c < ncat; ++c) {
                    double t = w[c] * L[c];
                    for (int32_t d = k[c] - kmin; d > 0; --d) t = t * kTreelikTiny;
                    post[(size_t)c * ncols + s] = t;
                    total = total + t;
                }
                site_l[s] = total;
                site_k[s] = kmin;
                for (uint32_t c = 0; c < ncat; ++c) post[(size_t)c * ncols + s] = post[(size_t)c * ncols + s] / total;
            }
        });

        parallel_for(ngroups * chunks_here, [&](size_t item) {
            const size_t group = item / chunks_here, chunk = chunk0 + item % chunks_here;
            const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
            std::vector<double> S(dim), Sv(dim), Em(dim), Ep(dim), Mm(dim), Mp(dim), X(dim), W(dim), T(dim);
            for (uint32_t at = group_off[group]; at < group_off[group + 1]; ++at) {
                const uint32_t q = order[at], v = cand_v[q], *node = &path[(size_t)q * PGM_TREELIK_SPR_STRIDE + 2];
                const uint32_t J = node[-2], M = node[-1], p = node[0], y = node[J + M];
                for (uint32_t s = s0; s < s1; ++s) {
                    double mixed = 0.0;
                    for (uint32_t k = 0; k < ncat; ++k) {
                        const double *Pk = P + pstride * k, *Phy = Ph + pstride * k + mat * y;
                        const double *Uk = &U[cstride * k + vstride * (s - site0)], *Ok = &O[cstride * k + vstride * (s - site0)];
                        auto apply = [&](const double *Z, uint32_t x, double *out) {   // Z the matrix of the edge above x
                            treelik_apply(Z, dim, x < nleaves ? nullptr : Uk + (size_t)(x - nleaves) * dim, x < nleaves ? (int)rows[(size_t)x * ncols + s] : 0, out);
                        };
                        // the - chain vector, and with `plus` the + one, times S_c of the children of node_at other than skip0 and skip1, in child order
                        auto others = [&](uint32_t node_at, uint32_t skip0, uint32_t skip1, bool plus) {
                            for (uint32_t r = ch.off[node_at]; r < ch.off[node_at + 1]; ++r) {
                                const uint32_t c = ch.idx[r];
                                if (c == skip0 || c == skip1) continue;
                                apply(Pk + mat * c, c, S.data());
                                for (uint32_t i = 0; i < dim; ++i) Em[i] = Em[i] * S[i];
                                for (uint32_t i = 0; plus && i < dim; ++i) Ep[i] = Ep[i] * S[i];
                            }
                        };
                        // out(i) = sum over h ascending of x(h) Z(h, i)
                        auto applied_from_above = [&](const double *Z, const double *x, double *out) {
                            for (uint32_t i = 0; i < dim; ++i) {
                                double acc = 0.0;
                                for (uint32_t h = 0; h < dim; ++h) acc = acc + x[h] * Z[h + (size_t)dim * i];
                                out[i] = acc;
                            }
                        };
                        int32_t km = 0, kp = 0;
                        auto rule = [&]() { km += treelik_rescale(Em.data(), dim) ? 1 : 0; kp += treelik_rescale(Ep.data(), dim) ? 1 : 0; };
                        apply(Pk + mat * v, v, Sv.data());
                        if (J >= 1 || M == 0) {   // the chain start
                            bool have = false;
                            for (uint32_t r = ch.off[p]; r < ch.off[p + 1]; ++r) {
                                const uint32_t c = ch.idx[r];
                                if (c == v) continue;
                                apply(Pk + mat * c, c, S.data());
                                for (uint32_t i = 0; i < dim; ++i) Em[i] = have ? Em[i] * S[i] : S[i];
                                have = true;
                            }
                            for (uint32_t i = 0; i < dim; ++i) Ep[i] = Em[i] * Sv[i];
                            rule();
                        }
                        for (uint32_t j = 1; j <= J; ++j) {   // up
                            treelik_apply(Pk + mat * node[j - 1], dim, Em.data(), 0, Mm.data());
                            treelik_apply(Pk + mat * node[j - 1], dim, Ep.data(), 0, Mp.data());
                            if (j < J || M == 0) {
                                Em = Mm; Ep = Mp;
                                others(node[j], node[j - 1], UINT32_MAX, true);
                                rule();
                            }
                        }
                        double N = 0.0, D = 0.0;
                        if (M == 0) {   // the target on the up chain
                            treelik_apply(Phy, dim, Em.data(), 0, X.data());
                            for (uint32_t i = 0; i < dim; ++i) X[i] = Sv[i] * X[i];
                            km += treelik_rescale(X.data(), dim) ? 1 : 0;
                            treelik_apply(Phy, dim, X.data(), 0, W.data());
                            treelik_apply(Pk + mat * y, dim, Ep.data(), 0, T.data());
                            const double *Oy = Ok + (size_t)(y - nleaves) * dim;
                            for (uint32_t h = 0; h < dim; ++h) { N = N + Oy[h] * W[h]; D = D + Oy[h] * T[h]; }
                        } else {
                            const uint32_t top = node[J];
                            if (top == root) for (uint32_t i = 0; i < dim; ++i) T[i] = pi[i];   // the turn: B_a
                            else applied_from_above(Pk + mat * top, Ok + (size_t)(top - nleaves) * dim, T.data());
                            if (J >= 1) {
                                for (uint32_t i = 0; i < dim; ++i) { Em[i] = T[i] * Mm[i]; Ep[i] = T[i] * Mp[i]; }
                                others(top, node[J - 1], node[J + 1], true);
                            } else {
                                Em = T;
                                others(top, v, node[J + 1], false);
                                for (uint32_t i = 0; i < dim; ++i) Ep[i] = Em[i] * Sv[i];
                            }
                            rule();
                            for (uint32_t m = 1; m < M; ++m) {   // down
                                applied_from_above(Pk + mat * node[J + m], Em.data(), Mm.data());
                                applied_from_above(Pk + mat * node[J + m], Ep.data(), Mp.data());
                                Em = Mm; Ep = Mp;
                                others(node[J + m], node[J + m + 1], UINT32_MAX, true);
                                rule();
                            }
                            apply(Phy, y, X.data());   // the target below the turn
                            for (uint32_t i = 0; i < dim; ++i) X[i] = Sv[i] * X[i];
                            km += treelik_rescale(X.data(), dim) ? 1 : 0;
                            treelik_apply(Phy, dim, X.data(), 0, W.data());
                            apply(Pk + mat * y, y, T.data());
                            for (uint32_t h = 0; h < dim; ++h) { N = N + Em[h] * W[h]; D = D + Ep[h] * T[h]; }
                        }
                        double r = 0.0;
                        if (D != 0.0) {
                            r = N / D;
                            for (int32_t d = km - kp; d > 0; --d) r = r * kTreelikTiny;
                            for (int32_t d = kp - km; d > 0; --d) r = r * kTreelikScale;
                        }
                        mixed = mixed + post[(size_t)k * ncols + s] * r;
                    }
                    rho[(size_t)q * ncols + s] = mixed;
                }
            }
        });
    }
}

void Backend::tree_spr(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                       const double *w, const double *P, const double *Ph, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_y, double *site_l, int32_t *site_k,
                       double *post, double *rho, int) {
    tree_spr_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, Ph, ncand, cand_v, cand_y, site_l, site_k, post, rho);
}

namespace {
std::vector<std::vector<uint32_t>> spr_children(uint32_t nnodes, const uint32_t *parent) {
    std::vector<std::vector<uint32_t>> kids(nnodes);
    for (uint32_t x = 0; x < nnodes; ++x)
        if (parent[x] != UINT32_MAX) kids[parent[x]].push_back(x);
    return kids;
}
}  // namespace

// The path of a candidate has as many edges as the tree has between p and y, so the targets of a prune node are the nodes within
// `radius` steps of p that are not reached through v: a breadth-first walk from p over parents and children.
void ml_spr_candidates(uint32_t nnodes, const uint32_t *parent, uint32_t radius, std::vector<uint32_t> &cand_v, std::vector<uint32_t> &cand_y) {
    cand_v.clear(); cand_y.clear();
    if (radius > PGM_TREE_SPR_MAXPATH) radius = PGM_TREE_SPR_MAXPATH;
    const std::vector<std::vector<uint32_t>> kids = spr_children(nnodes, parent);
    std::vector<uint32_t> dist(nnodes), seen(nnodes, UINT32_MAX), queue, targets;
    for (uint32_t v = 0; v + 1 < nnodes; ++v) {
        const uint32_t p = parent[v];
        const bool two = kids[p].size() == 2;
        if (two && parent[p] == UINT32_MAX) continue;
        queue.assign(1, p); targets.clear();
        seen[p] = v; dist[p] = 0; seen[v] = v;
        for (size_t at = 0; at < queue.size(); ++at) {
            const uint32_t x = queue[at];
            if (parent[x] != UINT32_MAX && !(two && (x == p || parent[x] == p))) targets.push_back(x);
            if (dist[x] == radius) continue;
            auto visit = [&](uint32_t z) { if (seen[z] != v) { seen[z] = v; dist[z] = dist[x] + 1; queue.push_back(z); } };
            if (parent[x] != UINT32_MAX) visit(parent[x]);
            for (uint32_t c : kids[x]) visit(c);
        }
        std::sort(targets.begin(), targets.end());
        for (uint32_t y : targets) { cand_v.push_back(v); cand_y.push_back(y); }
    }
}

std::vector<uint32_t> ml_spr_touched(uint32_t nnodes, const uint32_t *parent, uint32_t v, uint32_t y) {
    const uint32_t p = parent[v];
    std::vector<uint32_t> out = {v, p, y, parent[y]};
    if (parent[p] != UINT32_MAX) out.push_back(parent[p]);
    for (uint32_t x = 0; x < nnodes; ++x)
        if (parent[x] == p) out.push_back(x);
    for (uint32_t x = p, z = y; x != z;) {   // the path: both ends climb to the lowest common ancestor, the lower numbered first
        if (x < z) { out.push_back(x); x = parent[x]; }
        else { out.push_back(z); z = parent[z]; }
        if (x == z) out.push_back(x);
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

namespace {
struct SprTree {   // the nodes of topo and the new ones behind them; a dissolved node keeps its number and has no parent and no children
    std::vector<uint32_t> parent;
    std::vector<std::vector<uint32_t>> kids;
    std::vector<double> length;
};
PhyTree *spr_build(const MlTreeTopology &topo, const SprTree &t, uint32_t x) {
    std::unique_ptr<PhyTree> out(new PhyTree(x < topo.nleaves ? topo.names[x] : std::string()));
    for (uint32_t c : t.kids[x]) out->addChild(spr_build(topo, t, c), t.length[c], 1);
    return out.release();
}
}  // namespace

PhyTree *ml_spr_apply(const MlTreeTopology &topo, const std::vector<double> &lengths, uint32_t m, const uint32_t *move_v, const uint32_t *move_y) {
    SprTree t;
    t.parent = topo.parent;
    t.kids = spr_children(topo.nnodes, topo.parent.data());
    t.length = lengths;
    t.length.push_back(0.0);   // (the root's)
    auto replace = [&](uint32_t at, uint32_t old, uint32_t by) { *std::find(t.kids[at].begin(), t.kids[at].end(), old) = by; };
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t v = move_v[k], y = move_y[k], p = t.parent[v], above = t.parent[y], n = (uint32_t)t.parent.size();
        const double half = std::max(lengths[y] / 2, kMlMinLength);
        t.kids[p].erase(std::find(t.kids[p].begin(), t.kids[p].end(), v));
        t.parent.push_back(above); t.kids.push_back({y, v}); t.length.push_back(half);   // the new node in the middle of the edge above y
        replace(above, y, n);
        t.parent[y] = n; t.parent[v] = n;
        t.length[y] = half;
        if (t.kids[p].size() == 1) {   // p dissolves: its remaining child takes its place and the joined length
            const uint32_t s = t.kids[p][0];
            replace(t.parent[p], p, s);
            t.parent[s] = t.parent[p];
            t.length[s] = std::min(lengths[p] + lengths[s], kMlMaxLength);
            t.kids[p].clear();
            t.parent[p] = UINT32_MAX;
        }
    }
    return spr_build(topo, t, topo.nnodes - 1);
}

MlSprScan ml_spr_scan(const ModelFactory &mf, const MlTreeTopology &topo, const MlTreeResult &res, uint32_t ncols, const int8_t *rows, uint32_t radius, double eps,
                      Backend *be, size_t rho_bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    MlSprScan out;
    const uint32_t dim = (uint32_t)mf.dim(), nleaves = topo.nleaves, nnodes = topo.nnodes;
    std::vector<uint32_t> cv, cy;
    ml_spr_candidates(nnodes, topo.parent.data(), radius, cv, cy);
    const uint32_t ncand = (uint32_t)cv.size();
    out.candidates = ncand;
    if (ncand != 0) {
        const uint32_t ncat = res.rates.empty() ? 1u : (uint32_t)res.rates.size();
        const std::vector<double> w(ncat, res.rates.empty() ? 1.0 : 1.0 / (double)ncat);
        std::vector<double> halves(res.lengths.size()), P, Ph, site_l(ncols), post((size_t)ncat * ncols), rho, gain(ncand);
        std::vector<int32_t> site_k(ncols);
        for (size_t e = 0; e < halves.size(); ++e) halves[e] = std::max(res.lengths[e] / 2, kMlMinLength);
        if (res.rates.empty()) { treelik_matrices(mf, res.lengths, false, P); treelik_matrices(mf, halves, false, Ph); }
        else { treelik_matrices(mf, res.lengths, false, res.rates, P); treelik_matrices(mf, halves, false, res.rates, Ph); }
        // groups of whole prune nodes whose rho stays within rho_bytes (a prune node beyond that alone); every group is a call, which walks
        // the tree again (the entries are stateless)
        const size_t per_call = std::max<size_t>(1, rho_bytes / (8 * (size_t)ncols));
        for (uint32_t q0 = 0; q0 < ncand;) {
            uint32_t q1 = q0;
            while (q1 < ncand) {
                uint32_t next = q1;
                while (next < ncand && cv[next] == cv[q1]) ++next;
                if (q1 > q0 && next - q0 > per_call) break;
                q1 = next;
            }
            const uint32_t g = q1 - q0;
            rho.resize((size_t)g * ncols);
            if (be) be->tree_spr(dim, nleaves, nnodes, topo.parent.data(), ncols, rows, mf.freqs().data(), ncat, w.data(), P.data(), Ph.data(), g, cv.data() + q0, cy.data() + q0,
                                 site_l.data(), site_k.data(), post.data(), rho.data());
            else tree_spr_host(dim, nleaves, nnodes, topo.parent.data(), ncols, rows, mf.freqs().data(), ncat, w.data(), P.data(), Ph.data(), g, cv.data() + q0, cy.data() + q0,
                               site_l.data(), site_k.data(), post.data(), rho.data());
            ++ml_spr_stats.calls;
            parallel_for(g, [&](size_t q) { treelik_nni_gain(1, ncols, rho.data() + q * ncols, &gain[q0 + q]); });
            q0 = q1;
        }
        ml_spr_stats.candidates += ncand;
        out.best_gain = *std::max_element(gain.begin(), gain.end());
        std::vector<uint32_t> order;
        for (uint32_t q = 0; q < ncand; ++q)
            if (gain[q] > eps) order.push_back(q);
        out.positive = (uint32_t)order.size();
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return gain[x] > gain[y]; });
        std::vector<char> used(nnodes, 0);
        for (uint32_t q : order) {
            const std::vector<uint32_t> touched = ml_spr_touched(nnodes, topo.parent.data(), cv[q], cy[q]);
            if (std::any_of(touched.begin(), touched.end(), [&](uint32_t x) { return used[x] != 0; })) continue;
            for (uint32_t x : touched) used[x] = 1;
            out.pick_v.push_back(cv[q]); out.pick_y.push_back(cy[q]);
        }
    }
    ml_spr_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
}

}  // namespace pgm
