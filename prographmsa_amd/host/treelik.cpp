// treelik.cpp — the host parts of `pgmsa --ml_tree`: the host statement of
// pgm_tree_likelihood (Backend::tree_likelihood's default, what pgmsa_oracle runs), the matrices of every edge, the log-likelihood
// both drivers share, the numbering of a tree's nodes, and the optimiser of the branch lengths (and, with --ml_gamma, of the gamma's
// shape: treelik_rates.cpp has the categories' side).  The flow that writes the files is doMlTree in main.cpp.
//
// The arithmetic is Felsenstein pruning per site with both derivatives by every branch length.  Every sum runs over its index
// ascending from 0.0 with one multiply and one add per term, every product over the children in node order, and only + - * / occur:
// with -ffp-contract=off the loop below and the kernels of csrc/pgm_treelik_kernels.h give the same bits.
#include "treelik_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>

namespace pgm {

MlTreeStats ml_tree_stats;

void tree_likelihood_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                          const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2) {
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, derivs, site_l, site_k, d1, d2);
    const uint32_t nedges = nnodes - 1;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk;
    std::vector<double> c1, c2;   // per chunk and edge: the sums of g and h over the chunk's sites, ascending
    if (derivs) { c1.assign(nchunks * nedges, 0.0); c2.assign(nchunks * nedges, 0.0); }

    parallel_for(nchunks, [&](size_t chunk) {
        TreelikSiteWalk walk(ch, dim, nleaves, nnodes, ncols, rows, pi, derivs != 0);
        std::vector<double> g(nedges), q(nedges);
        const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
        for (uint32_t s = s0; s < s1; ++s) {
            walk(s, P, site_l[s], site_k[s], g.data(), q.data());
            if (!derivs) continue;
            for (uint32_t e = 0; e < nedges; ++e) {
                c1[chunk * nedges + e] = c1[chunk * nedges + e] + g[e];
                c2[chunk * nedges + e] = c2[chunk * nedges + e] + (q[e] - g[e] * g[e]);
            }
        }
    });
    if (!derivs) return;
    treelik_chunk_totals(c1, c2, nchunks, nedges, d1, d2);
}

void Backend::tree_likelihood(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                              const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2, int) {
    tree_likelihood_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, derivs, site_l, site_k, d1, d2);
}

void treelik_matrices(const ModelFactory &mf, const std::vector<double> &t, bool derivs, std::vector<double> &P) {
    const size_t n = (size_t)mf.dim(), mat = n * n, stride = derivs ? 3 * mat : mat;
    const std::vector<double> &Q = mf.Qmat();
    P.resize(stride * t.size());
    parallel_for(t.size(), [&](size_t e) {
        double *Pe = &P[stride * e];
        const std::vector<double> p = mf.transition(t[e]);
        std::copy(p.begin(), p.end(), Pe);
        for (int x = 1; derivs && x < 3; ++x) {   // Q P, then Q (Q P)
            const double *src = Pe + mat * (x - 1);
            double *dst = Pe + mat * x;
            for (size_t j = 0; j < n; ++j)
                for (size_t i = 0; i < n; ++i) {
                    double acc = 0.0;
                    for (size_t k = 0; k < n; ++k) acc = acc + Q[i + n * k] * src[k + n * j];
                    dst[i + n * j] = acc;
                }
        }
    });
}

double treelik_lnl(uint32_t ncols, const double *site_l, const int32_t *site_k, double *site_lnl) {
    const double step = 256.0 * std::log(2.0);
    double lnl = 0.0;
    for (uint32_t s = 0; s < ncols; ++s) {
        const double v = std::log(site_l[s]) - (double)site_k[s] * step;
        if (site_lnl) site_lnl[s] = v;
        lnl = lnl + v;
    }
    return lnl;
}

MlTreeTopology ml_tree_topology(const PhyTree &tree) {
    MlTreeTopology topo;
    const LeafNumbering num = leaf_numbering(tree);
    if (num.nleaves < 2 || num.nleaves > 0x7fffffffull) error("ml tree: a tree of %zu leaves", num.nleaves);
    topo.nleaves = (uint32_t)num.nleaves;
    topo.names.resize(num.nleaves);
    for (const auto &kv : num.index) topo.names[kv.second] = kv.first;
    topo.node.assign(num.nleaves, nullptr);
    topo.parent.assign(num.nleaves, UINT32_MAX);
    std::function<uint32_t(const PhyTree &)> walk = [&](const PhyTree &t) -> uint32_t {
        if (t.isLeaf()) {
            const uint32_t id = (uint32_t)num.index.at(t.getName());
            if (topo.node[id]) error("ml tree: leaf %s twice", t.getName().c_str());
            topo.node[id] = &t;
            return id;
        }
        if (t.n_children() < 2) error("ml tree: an inner node with one child");
        std::vector<uint32_t> kids;
        for (index_t c = 0; c < t.n_children(); ++c) kids.push_back(walk(t[(int)c]));
        const uint32_t id = (uint32_t)topo.node.size();
        topo.node.push_back(&t);
        topo.parent.push_back(UINT32_MAX);
        for (uint32_t c : kids) topo.parent[c] = id;
        return id;
    };
    if (tree.isLeaf()) error("ml tree: a tree of one leaf");
    walk(tree);
    topo.nnodes = (uint32_t)topo.node.size();
    return topo;
}

PhyTree *ml_tree_with_lengths(const MlTreeTopology &topo, const std::vector<double> &lengths) {
    std::map<const PhyTree *, uint32_t> id;
    for (uint32_t v = 0; v < topo.nnodes; ++v) id[topo.node[v]] = v;
    std::function<PhyTree *(const PhyTree &)> build = [&](const PhyTree &t) -> PhyTree * {
        std::unique_ptr<PhyTree> out(new PhyTree(t.getName()));
        for (index_t c = 0; c < t.n_children(); ++c) {
            const PhyTree &kid = t[(int)c];
            out->addChild(build(kid), lengths[id.at(&kid)], kid.getBranchSupport());
        }
        return out.release();
    };
    return build(*topo.node[topo.nnodes - 1]);
}

MlTreeResult ml_branch_lengths(const Alphabet &a, const std::vector<std::vector<int8_t>> &rows, const ModelFactory &model_factory, const PhyTree &tree,
                               uint32_t rounds, double eps, Backend *be, const MlGamma &gamma) {
    const auto t0 = std::chrono::steady_clock::now();
    const MlTreeTopology topo = ml_tree_topology(tree);
    const uint32_t dim = (uint32_t)model_factory.dim(), nleaves = topo.nleaves, nnodes = topo.nnodes, nedges = nnodes - 1;
    if ((int)dim != a.DIM) error("ml tree: a model of %u states for an alphabet of %d", dim, a.DIM);
    if (rows.size() != nleaves) error("ml tree: %zu rows for a tree of %u leaves", rows.size(), nleaves);
    const size_t L = rows[0].size();
    if (L == 0 || L > 0x7fffffffull) error("ml tree: an alignment of %zu columns", L);
    const uint32_t ncols = (uint32_t)L;
    std::vector<int8_t> flat((size_t)nleaves * ncols);
    for (uint32_t r = 0; r < nleaves; ++r) {
        if (rows[r].size() != L) error("ml tree: rows of different lengths");
        std::copy(rows[r].begin(), rows[r].end(), flat.begin() + (size_t)r * ncols);
    }
    auto clamp = [](double t) { return !(t > kMlMinLength) ? kMlMinLength : t > kMlMaxLength ? kMlMaxLength : t; };   // (a NaN: the lower bound)
    const uint32_t ncat = gamma.ncat >= 2 ? gamma.ncat : 0;   // 0: one rate, the entry without categories
    if (ncat > PGM_TREELIK_MAXCAT) error("ml tree: %u rate categories", ncat);

    MlTreeResult res;
    std::vector<double> t(nedges), P, site_l(ncols), trial_l(ncols), d1(nedges), d2(nedges), target(nedges), trial(nedges);
    std::vector<int32_t> site_k(ncols), trial_k(ncols);
    std::vector<double> rates, post((size_t)ncat * ncols), trial_post(post.size());   // (with categories only)
    const std::vector<double> weights(ncat, ncat ? 1.0 / (double)ncat : 0.0);
    double alpha = gamma.estimate ? gamma.start : gamma.alpha;
    if (ncat) rates = gamma_rates(alpha, ncat);
    for (uint32_t e = 0; e < nedges; ++e) t[e] = clamp(topo.node[e]->getBranchLength());
    const double *pi = model_factory.freqs().data();
    // lnL at the lengths `at` (and the categories' rates `r`): the site values into l, k (and pp), with derivs d1 and d2
    auto evaluate = [&](const std::vector<double> &at, const std::vector<double> &r, bool derivs, double *l, int32_t *k, double *pp) {
        if (ncat) {
            treelik_matrices(model_factory, at, derivs, r, P);
            if (be) be->tree_likelihood_rates(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, ncat, weights.data(), P.data(), derivs ? 1 : 0, l, k, pp, d1.data(), d2.data());
            else tree_likelihood_rates_host(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, ncat, weights.data(), P.data(), derivs ? 1 : 0, l, k, pp, d1.data(), d2.data());
        } else {
            treelik_matrices(model_factory, at, derivs, P);
            if (be) be->tree_likelihood(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, P.data(), derivs ? 1 : 0, l, k, d1.data(), d2.data());
            else tree_likelihood_host(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, P.data(), derivs ? 1 : 0, l, k, d1.data(), d2.data());
        }
        ++res.evaluations;
        return treelik_lnl(ncols, l, k, nullptr);
    };
    double lnl = 0;
    bool started = false;
    // the branch-length loop at the rates in hand, until it stops by its own rules
    auto branch_lengths = [&]() {
        for (uint32_t round = 0; round < rounds; ++round) {
            const double here = evaluate(t, rates, true, site_l.data(), site_k.data(), post.data());   // (the up pass of the accepted point again: the same bits)
            if (!started) { res.lnl_start = here; started = true; }
            lnl = here;
            ++res.rounds;
            for (uint32_t e = 0; e < nedges; ++e)
                target[e] = clamp(d2[e] < 0 ? t[e] - d1[e] / d2[e] : d1[e] > 0 ? 2 * t[e] : t[e] / 2);
            bool accepted = false;
            double gain = 0, lambda = 1.0;
            for (int step = 0; step <= 10 && !accepted; ++step, lambda *= 0.5) {
                for (uint32_t e = 0; e < nedges; ++e) trial[e] = clamp(t[e] + lambda * (target[e] - t[e]));
                const double there = evaluate(trial, rates, false, trial_l.data(), trial_k.data(), trial_post.data());
                if (there > lnl) { accepted = true; gain = there - lnl; lnl = there; }
            }
            if (!accepted) break;
            t.swap(trial); site_l.swap(trial_l); site_k.swap(trial_k); post.swap(trial_post);
            if (gain < eps) break;
        }
    };
    if (!ncat || !gamma.estimate) branch_lengths();
    else {
        // the loop above and a golden-section search on x = ln alpha in turns.  The search: kMlAlphaEvaluations evaluations without
        // derivatives inside [x - W / 2, x + W / 2] cut to [ln kMlMinAlpha, ln kMlMaxAlpha], W the whole range in the first pair and a
        // quarter of the previous W in every later one; its best point is taken only if its lnL is strictly above the one in hand
        const double x_lo = std::log(kMlMinAlpha), x_hi = std::log(kMlMaxAlpha), ratio = (std::sqrt(5.0) - 1.0) / 2.0;
        double width = x_hi - x_lo;
        std::vector<double> best_l(ncols), best_post(post.size());
        std::vector<int32_t> best_k(ncols);
        for (uint32_t pair = 0; pair < kMlMaxPairs; ++pair, width *= 0.25) {
            const double before = pair == 0 ? -INFINITY : lnl;
            branch_lengths();
            const double x = std::log(alpha);
            double lo = pair == 0 ? x_lo : std::max(x_lo, x - width / 2), hi = pair == 0 ? x_hi : std::min(x_hi, x + width / 2);
            double best = lnl, best_x = x;
            bool found = false;
            auto probe = [&](double at) {
                const double v = evaluate(t, gamma_rates(std::exp(at), ncat), false, trial_l.data(), trial_k.data(), trial_post.data());
                if (v > best) { best = v; best_x = at; found = true; best_l.swap(trial_l); best_k.swap(trial_k); best_post.swap(trial_post); }
                return v;
            };
            double x1 = hi - ratio * (hi - lo), x2 = lo + ratio * (hi - lo), f1 = probe(x1), f2 = probe(x2);
            for (uint32_t n = 2; n < kMlAlphaEvaluations; ++n) {
                if (f1 < f2) { lo = x1; x1 = x2; f1 = f2; x2 = lo + ratio * (hi - lo); f2 = probe(x2); }
                else { hi = x2; x2 = x1; f2 = f1; x1 = hi - ratio * (hi - lo); f1 = probe(x1); }
            }
            if (found) {
                alpha = std::exp(best_x);           // (a point strictly inside the range)
                rates = gamma_rates(alpha, ncat);   // (the rates the probe had: the site values in hand are those of (t, alpha))
                lnl = best;
                site_l.swap(best_l); site_k.swap(best_k); post.swap(best_post);
            }
            if (!found || lnl - before < eps) break;
        }
    }
    res.lengths = t;
    res.lnl = lnl;
    res.site_lnl.resize(ncols);
    (void)treelik_lnl(ncols, site_l.data(), site_k.data(), res.site_lnl.data());
    if (ncat) { res.alpha = alpha; res.rates = rates; res.post = post; ml_tree_stats.categories = ncat; ml_tree_stats.alpha = alpha; }
    ml_tree_stats.rounds += res.rounds; ml_tree_stats.evaluations += res.evaluations;
    ml_tree_stats.lnl_start = res.lnl_start; ml_tree_stats.lnl = res.lnl;
    ml_tree_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return res;
}

}  // namespace pgm
