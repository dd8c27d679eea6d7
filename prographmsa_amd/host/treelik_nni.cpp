// treelik_nni.cpp — nearest-neighbour interchanges for `pgmsa --ml_tree --ml_search` (the walk and the checks are
// treelik_internal.h's): the host statement of pgm_tree_nni (Backend::tree_nni's
// default, what pgmsa_oracle runs), the gain of a candidate both drivers share, and the topology search, which is host code and the
// same for every backend.
#include "treelik_internal.h"

#include <chrono>

namespace pgm {

MlSearchStats ml_search_stats;

void tree_nni_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                   const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, double *site_l,
                   int32_t *site_k, double *post, double *rho, size_t block_bytes) {
    if (!w || !post || !cand_v || !cand_a || !cand_c || !rho) error("tree likelihood: null argument");
    treelik_check_rates_host(ncat, w);
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, 0, site_l, site_k, nullptr, nullptr);
    const std::string bad = pgm_treelik_check_candidates(nleaves, nnodes, parent, ncand, cand_v, cand_a, cand_c);
    if (!bad.empty()) error("%s", bad.c_str());
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves, root = nnodes - 1;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk, mat = (size_t)dim * dim, pstride = mat * nedges;
    // The partials and the outside vectors are kept for a block of column chunks at a time, [category][site of the block][inner node]
    // [state], so that what is held stays near block_bytes whatever the alignment's width: per block the walk of every
    // category and site on the host threads, then the candidates as a parallel_for over candidates x column chunks of the block.
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

        // the candidates: independent of each other and of the columns
        parallel_for((size_t)ncand * chunks_here, [&](size_t item) {
            const uint32_t q = (uint32_t)(item / chunks_here), v = cand_v[q], a = cand_a[q], c = cand_c[q], u = parent[v];
            const size_t chunk = chunk0 + item % chunks_here;
            const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
            std::vector<double> S(dim), R(dim), T(dim), Sa(dim), Sc(dim), X(dim), Y(dim);
            for (uint32_t s = s0; s < s1; ++s) {
                double mixed = 0.0;
                for (uint32_t k = 0; k < ncat; ++k) {
                    const double *Pk = P + pstride * k, *Uk = &U[cstride * k + vstride * (s - site0)], *Ok = &O[cstride * k + vstride * (s - site0)];
                    auto apply = [&](uint32_t x, double *out) {
                        treelik_apply(Pk + mat * x, dim, x < nleaves ? nullptr : Uk + (size_t)(x - nleaves) * dim, x < nleaves ? (int)rows[(size_t)x * ncols + s] : 0, out);
                    };
                    if (u == root) for (uint32_t i = 0; i < dim; ++i) R[i] = pi[i];
                    else {
                        const double *Ou = Ok + (size_t)(u - nleaves) * dim, *Pu = Pk + mat * u;
                        for (uint32_t i = 0; i < dim; ++i) {
                            double acc = 0.0;
                            for (uint32_t h = 0; h < dim; ++h) acc = acc + Ou[h] * Pu[h + (size_t)dim * i];
                            R[i] = acc;
                        }
                    }
                    for (uint32_t r = ch.off[u]; r < ch.off[u + 1]; ++r) {
                        const uint32_t sib = ch.idx[r];
                        if (sib == v || sib == c) continue;
                        apply(sib, S.data());
                        for (uint32_t i = 0; i < dim; ++i) R[i] = R[i] * S[i];
                    }
                    bool have = false;
                    for (uint32_t r = ch.off[v]; r < ch.off[v + 1]; ++r) {
                        const uint32_t b = ch.idx[r];
                        if (b == a) continue;
                        apply(b, S.data());
                        for (uint32_t i = 0; i < dim; ++i) T[i] = have ? T[i] * S[i] : S[i];
                        have = true;
                    }
                    apply(a, Sa.data());
                    apply(c, Sc.data());
                    double A[2];
                    int32_t count[2];
                    for (int side = 0; side < 2; ++side) {   // the tree as it is, then the neighbour
                        const double *Sx = side == 0 ? Sa.data() : Sc.data(), *Sy = side == 0 ? Sc.data() : Sa.data();
                        for (uint32_t i = 0; i < dim; ++i) { X[i] = T[i] * Sx[i]; Y[i] = R[i] * Sy[i]; }
                        count[side] = (treelik_rescale(X.data(), dim) ? 1 : 0) + (treelik_rescale(Y.data(), dim) ? 1 : 0);
                        treelik_apply(Pk + mat * v, dim, X.data(), 0, S.data());   // W
                        double acc = 0.0;
                        for (uint32_t i = 0; i < dim; ++i) acc = acc + Y[i] * S[i];
                        A[side] = acc;
                    }
                    double r = 0.0;
                    if (A[0] != 0.0) {
                        r = A[1] / A[0];
                        for (int32_t d = count[1] - count[0]; d > 0; --d) r = r * kTreelikTiny;
                        for (int32_t d = count[0] - count[1]; d > 0; --d) r = r * kTreelikScale;
                    }
                    mixed = mixed + post[(size_t)k * ncols + s] * r;
                }
                rho[(size_t)q * ncols + s] = mixed;
            }
        });
    }
}

void Backend::tree_nni(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                       const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, double *site_l,
                       int32_t *site_k, double *post, double *rho, int) {
    tree_nni_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cand_v, cand_a, cand_c, site_l, site_k, post, rho);
}

void treelik_nni_gain(uint32_t ncand, uint32_t ncols, const double *rho, double *gain) {
    for (uint32_t q = 0; q < ncand; ++q) {
        double acc = 0.0;
        for (uint32_t s = 0; s < ncols; ++s) acc = acc + std::log(rho[(size_t)q * ncols + s]);   // (log 0 is -infinity)
        gain[q] = acc;
    }
}

namespace {
// a tree as the search holds it: the numbering of ml_tree_topology, the children of every node in ascending order, the length above
// every node
struct MlSearchTree {
    uint32_t nleaves = 0, nnodes = 0;
    std::vector<std::string> names;
    std::vector<std::vector<uint32_t>> kids;
    std::vector<double> length;
    uint32_t root = 0;
};
MlSearchTree ml_search_tree(const MlTreeTopology &topo, const std::vector<double> &lengths) {
    MlSearchTree t;
    t.nleaves = topo.nleaves; t.nnodes = topo.nnodes; t.names = topo.names; t.root = topo.nnodes - 1;
    t.kids.resize(topo.nnodes);
    for (uint32_t v = 0; v + 1 < topo.nnodes; ++v) t.kids[topo.parent[v]].push_back(v);
    t.length = lengths;
    t.length.push_back(0.0);
    return t;
}
PhyTree *ml_search_build(const MlSearchTree &t, uint32_t v) {
    std::unique_ptr<PhyTree> out(new PhyTree(v < t.nleaves ? t.names[v] : std::string()));
    for (uint32_t c : t.kids[v]) out->addChild(ml_search_build(t, c), t.length[c], 1);
    return out.release();
}
}  // namespace

MlSearchResult ml_topology_search(const Alphabet &a, const std::vector<std::vector<int8_t>> &rows, const ModelFactory &model_factory, const PhyTree &start,
                                  uint32_t search_rounds, uint32_t rounds, double eps, Backend *be, const MlGamma &gamma) {
    const auto t0 = std::chrono::steady_clock::now();
    MlSearchResult out;
    out.tree.reset(start.copy());
    out.res = ml_branch_lengths(a, rows, model_factory, *out.tree, rounds, eps, be, gamma);
    const double lnl_start = out.res.lnl_start;
    const uint32_t dim = (uint32_t)model_factory.dim(), ncols = (uint32_t)rows[0].size();
    std::vector<int8_t> flat;
    for (const auto &r : rows) flat.insert(flat.end(), r.begin(), r.end());
    const double *pi = model_factory.freqs().data();

    for (uint32_t round = 1; round <= search_rounds; ++round) {
        const MlTreeTopology topo = ml_tree_topology(*out.tree);
        const uint32_t nleaves = topo.nleaves, nnodes = topo.nnodes;
        const MlSearchTree cur = ml_search_tree(topo, out.res.lengths);
        // the candidates: v ascending, a in child order, c in child order
        std::vector<uint32_t> cv, ca, cc;
        for (uint32_t v = nleaves; v + 1 < nnodes; ++v)
            for (uint32_t x : cur.kids[v])
                for (uint32_t y : cur.kids[topo.parent[v]])
                    if (y != v) { cv.push_back(v); ca.push_back(x); cc.push_back(y); }
        MlSearchRound line;
        line.round = round; line.candidates = (uint32_t)cv.size();
        line.lnl_before = line.lnl_applied = line.lnl_after = out.res.lnl;
        if (cv.empty()) { out.log.push_back(line); break; }   // (a tree whose root alone is an inner node)
        const uint32_t ncand = (uint32_t)cv.size();
        const uint32_t ncat = out.res.rates.empty() ? 1u : (uint32_t)out.res.rates.size();
        const std::vector<double> w(ncat, out.res.rates.empty() ? 1.0 : 1.0 / (double)ncat);
        std::vector<double> P, site_l(ncols), post((size_t)ncat * ncols), rho((size_t)ncand * ncols), gain(ncand);
        std::vector<int32_t> site_k(ncols);
        if (out.res.rates.empty()) treelik_matrices(model_factory, out.res.lengths, false, P);
        else treelik_matrices(model_factory, out.res.lengths, false, out.res.rates, P);
        if (be) be->tree_nni(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), ncand, cv.data(), ca.data(), cc.data(), site_l.data(),
                             site_k.data(), post.data(), rho.data());
        else tree_nni_host(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), ncand, cv.data(), ca.data(), cc.data(), site_l.data(),
                           site_k.data(), post.data(), rho.data());
        ++ml_search_stats.calls;
        treelik_nni_gain(ncand, ncols, rho.data(), gain.data());
        line.best_gain = *std::max_element(gain.begin(), gain.end());
        // the candidates above the threshold by gain descending, then by index; picked greedily while they share no node
        std::vector<uint32_t> order;
        for (uint32_t q = 0; q < ncand; ++q)
            if (gain[q] > eps) order.push_back(q);
        line.positive = (uint32_t)order.size();
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return gain[x] > gain[y]; });
        std::vector<char> used(nnodes, 0);
        std::vector<uint32_t> picked;
        for (uint32_t q : order) {
            const uint32_t four[4] = {topo.parent[cv[q]], cv[q], ca[q], cc[q]};
            if (used[four[0]] || used[four[1]] || used[four[2]] || used[four[3]]) continue;
            for (uint32_t x : four) used[x] = 1;
            picked.push_back(q);
        }
        if (picked.empty()) { out.log.push_back(line); break; }
        bool accepted = false;
        for (size_t m = picked.size(); m >= 1 && !accepted; m = m / 2) {
            MlSearchTree next = cur;
            for (size_t p = 0; p < m; ++p) {   // a and c exchanged: both keep their length, each takes the other's place among the children
                const uint32_t q = picked[p], v = cv[q], u = topo.parent[v];
                *std::find(next.kids[v].begin(), next.kids[v].end(), ca[q]) = cc[q];
                *std::find(next.kids[u].begin(), next.kids[u].end(), cc[q]) = ca[q];
            }
            std::unique_ptr<PhyTree> tree(ml_search_build(next, next.root));
            // one evaluation without derivatives at the carried lengths and the rates in hand (ml_tree_topology numbers the new tree)
            const MlTreeTopology nt = ml_tree_topology(*tree);
            std::vector<double> t(nt.nnodes - 1);
            for (uint32_t e = 0; e + 1 < nt.nnodes; ++e) t[e] = nt.node[e]->getBranchLength();
            if (out.res.rates.empty()) {
                treelik_matrices(model_factory, t, false, P);
                if (be) be->tree_likelihood(dim, nleaves, nnodes, nt.parent.data(), ncols, flat.data(), pi, P.data(), 0, site_l.data(), site_k.data(), nullptr, nullptr);
                else tree_likelihood_host(dim, nleaves, nnodes, nt.parent.data(), ncols, flat.data(), pi, P.data(), 0, site_l.data(), site_k.data(), nullptr, nullptr);
            } else {
                treelik_matrices(model_factory, t, false, out.res.rates, P);
                if (be) be->tree_likelihood_rates(dim, nleaves, nnodes, nt.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), 0, site_l.data(), site_k.data(),
                                                  post.data(), nullptr, nullptr);
                else tree_likelihood_rates_host(dim, nleaves, nnodes, nt.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), 0, site_l.data(), site_k.data(),
                                                post.data(), nullptr, nullptr);
            }
            ++ml_tree_stats.evaluations;
            const double there = treelik_lnl(ncols, site_l.data(), site_k.data(), nullptr);
            if (there > line.lnl_before) {
                accepted = true;
                line.applied = (uint32_t)m;
                line.lnl_applied = there;
                MlGamma from = gamma;
                if (gamma.ncat >= 2 && gamma.estimate) from.start = out.res.alpha;
                out.tree = std::move(tree);
                out.res = ml_branch_lengths(a, rows, model_factory, *out.tree, rounds, eps, be, from);
                line.lnl_after = out.res.lnl;
            }
        }
        out.log.push_back(line);
        if (!accepted) break;
        ++ml_search_stats.rounds;
        ml_search_stats.applied += line.applied;
    }
    out.res.lnl_start = lnl_start;
    ml_tree_stats.lnl_start = lnl_start;
    ml_search_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
}

}  // namespace pgm
