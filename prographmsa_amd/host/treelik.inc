// treelik.inc — the host parts of `pgmsa --ml_tree` (included by model_factory.cpp; DESIGN.md 3.17): the host statement of
// pgm_tree_likelihood (Backend::tree_likelihood's default, what pgmsa_oracle runs), the matrices of every edge, the log-likelihood
// both drivers share, the numbering of a tree's nodes, and the optimiser of the branch lengths (and, with --ml_gamma, of the gamma's
// shape: treelik_rates.inc has the categories' side, DESIGN.md 3.18).  The flow that writes the files is doMlTree in main.cpp.
//
// The arithmetic is Felsenstein pruning per site with both derivatives by every branch length.  Every sum runs over its index
// ascending from 0.0 with one multiply and one add per term, every product over the children in node order, and only + - * / occur:
// with -ffp-contract=off the loop below and the kernels of csrc/pgm_treelik_kernels.h give the same bits.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>

namespace pgm {

MlTreeStats ml_tree_stats;

namespace {
const double kTreelikTiny = 0x1p-256, kTreelikScale = 0x1p256;
const uint32_t kTreelikChunk = PGM_TREELIK_CHUNK;

// the children of every node in ascending order (CSR), after the checks of the C entry (include/pgm_hip.h: pgm_tree_likelihood)
struct TreelikChildren { std::vector<uint32_t> off, idx; };
TreelikChildren treelik_check_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                   const double *P, int derivs, const double *site_l, const int32_t *site_k, const double *d1, const double *d2) {
    if (!parent || !rows || !pi || !P || !site_l || !site_k || (derivs && (!d1 || !d2))) error("tree likelihood: null argument");
    if (dim < 1 || dim > 64) error("tree likelihood: dim must be 1 .. 64");
    if (nleaves < 2 || ncols == 0 || nnodes <= nleaves) error("tree likelihood: nleaves must be at least 2, ncols at least 1 and nnodes above nleaves");
    TreelikChildren ch;
    ch.off.assign((size_t)nnodes + 1, 0);
    uint32_t roots = 0;
    for (uint32_t v = 0; v < nnodes; ++v) {
        if (parent[v] == UINT32_MAX) { ++roots; continue; }
        if (parent[v] <= v || parent[v] >= nnodes) error("tree likelihood: the parent of node %u is not above it", v);
        if (parent[v] < nleaves) error("tree likelihood: leaf %u is a parent", parent[v]);
        ++ch.off[parent[v] + 1];
    }
    if (roots != 1) error("tree likelihood: %u roots", roots);
    for (uint32_t v = nleaves; v < nnodes; ++v)
        if (ch.off[v + 1] < 2) error("tree likelihood: inner node %u has fewer than 2 children", v);
    for (uint32_t v = 0; v < nnodes; ++v) ch.off[v + 1] += ch.off[v];
    ch.idx.resize(ch.off[nnodes]);
    std::vector<uint32_t> fill(ch.off.begin(), ch.off.end() - 1);
    for (uint32_t v = 0; v < nnodes; ++v)
        if (parent[v] != UINT32_MAX) ch.idx[fill[parent[v]]++] = v;
    for (size_t k = 0; k < (size_t)nleaves * ncols; ++k)
        if (rows[k] < -2 || rows[k] >= (int)dim) error("tree likelihood: row value %d outside -2 .. dim - 1", (int)rows[k]);
    return ch;
}

// out(i) = sum over j ascending of X(i, j) u(j), u the partial of a child: `u` for an inner node, for a leaf the indicator of its
// value r (r < 0: ones).  A leaf with a state: 0.0 + X(i, r), what the sum gives when every other term is a zero.
inline void treelik_apply(const double *X, uint32_t dim, const double *u, int r, double *out) {
    if (!u && r >= 0) {
        for (uint32_t i = 0; i < dim; ++i) out[i] = 0.0 + X[i + (size_t)dim * (uint32_t)r];
        return;
    }
    for (uint32_t i = 0; i < dim; ++i) out[i] = 0.0;
    for (uint32_t j = 0; j < dim; ++j) {
        const double uj = u ? u[j] : 1.0;
        const double *col = X + (size_t)dim * j;
        for (uint32_t i = 0; i < dim; ++i) out[i] = out[i] + col[i] * uj;
    }
}
// the scaling rule: a vector whose largest entry is below 2^-256 and above 0 is multiplied by 2^256
inline bool treelik_rescale(double *v, uint32_t dim) {
    double m = v[0];
    for (uint32_t i = 1; i < dim; ++i) m = v[i] > m ? v[i] : m;
    if (!(m < kTreelikTiny && m > 0.0)) return false;
    for (uint32_t i = 0; i < dim; ++i) v[i] = v[i] * kTreelikScale;
    return true;
}
// d1[e], d2[e]: the chunk sums of edge e, chunks ascending
inline void treelik_chunk_totals(const std::vector<double> &c1, const std::vector<double> &c2, size_t nchunks, uint32_t nedges, double *d1, double *d2) {
    for (uint32_t e = 0; e < nedges; ++e) {
        double a1 = 0.0, a2 = 0.0;
        for (size_t chunk = 0; chunk < nchunks; ++chunk) { a1 = a1 + c1[chunk * nedges + e]; a2 = a2 + c2[chunk * nedges + e]; }
        d1[e] = a1;
        d2[e] = a2;
    }
}

// The walk over the tree for one site at a time, with the scratch of one thread: the up pass, the scaling rule, and with derivs the
// down pass and the three sums of every edge.  The host statements are loops over it.  posteriors() is the down pass of
// tree_ancestral_host (treelik_anc.inc): a walk made with derivs == false and anc == true.
struct TreelikSiteWalk {
    const TreelikChildren &ch;
    uint32_t dim, nleaves, nnodes, ncols;
    const int8_t *rows;
    const double *pi;
    bool derivs;
    std::vector<double> U, O, S, base, o, T;
    TreelikSiteWalk(const TreelikChildren &ch_, uint32_t dim_, uint32_t nleaves_, uint32_t nnodes_, uint32_t ncols_, const int8_t *rows_, const double *pi_, bool derivs_,
                    bool anc = false)
        : ch(ch_), dim(dim_), nleaves(nleaves_), nnodes(nnodes_), ncols(ncols_), rows(rows_), pi(pi_), derivs(derivs_) {
        uint32_t max_kids = 2;
        for (uint32_t v = nleaves; v < nnodes; ++v) max_kids = std::max(max_kids, ch.off[v + 1] - ch.off[v]);
        const size_t ninner = nnodes - nleaves;
        U.resize(ninner * dim); O.resize(derivs || anc ? ninner * dim : 0); S.resize((size_t)max_kids * dim); base.resize(dim); o.resize(dim); T.resize(3 * (size_t)dim);
    }
    // site s under the matrices P: (L, k), and with derivs g[e] = A^P' / A^P and q[e] = A^P'' / A^P of every edge e
    void operator()(uint32_t s, const double *P, double &L_out, int32_t &k_out, double *g, double *q) {
        const uint32_t root = nnodes - 1;
        const size_t mat = (size_t)dim * dim, estride = derivs ? 3 * mat : mat;
        auto partial = [&](uint32_t c) -> const double * { return c < nleaves ? nullptr : &U[(size_t)(c - nleaves) * dim]; };
        auto value = [&](uint32_t c) -> int { return c < nleaves ? (int)rows[(size_t)c * ncols + s] : 0; };
        // up pass
        int32_t k = 0;
        for (uint32_t v = nleaves; v < nnodes; ++v) {
            double *Uv = &U[(size_t)(v - nleaves) * dim];
            for (uint32_t qq = ch.off[v]; qq < ch.off[v + 1]; ++qq) {
                const uint32_t c = ch.idx[qq];
                treelik_apply(P + estride * c, dim, partial(c), value(c), S.data());
                if (qq == ch.off[v]) for (uint32_t i = 0; i < dim; ++i) Uv[i] = S[i];
                else for (uint32_t i = 0; i < dim; ++i) Uv[i] = Uv[i] * S[i];
            }
            if (treelik_rescale(Uv, dim)) ++k;
        }
        double L = 0.0;
        for (uint32_t i = 0; i < dim; ++i) L = L + pi[i] * U[(size_t)(root - nleaves) * dim + i];
        L_out = L;
        k_out = k;
        if (!derivs) return;
        // down pass: the outside vector of every edge, then the three sums of the edge
        for (uint32_t v = root; v >= nleaves; --v) {
            if (v == root) for (uint32_t i = 0; i < dim; ++i) base[i] = pi[i];
            else {
                const double *Ov = &O[(size_t)(v - nleaves) * dim], *Pv = P + estride * v;
                for (uint32_t i = 0; i < dim; ++i) {
                    double acc = 0.0;
                    for (uint32_t h = 0; h < dim; ++h) acc = acc + Ov[h] * Pv[h + (size_t)dim * i];
                    base[i] = acc;
                }
            }
            const uint32_t q0 = ch.off[v], q1 = ch.off[v + 1];
            for (uint32_t qq = q0; qq < q1; ++qq) treelik_apply(P + estride * ch.idx[qq], dim, partial(ch.idx[qq]), value(ch.idx[qq]), &S[(size_t)(qq - q0) * dim]);
            for (uint32_t qq = q0; qq < q1; ++qq) {
                const uint32_t c = ch.idx[qq];
                for (uint32_t i = 0; i < dim; ++i) o[i] = base[i];
                for (uint32_t r = q0; r < q1; ++r)
                    if (r != qq) for (uint32_t i = 0; i < dim; ++i) o[i] = o[i] * S[(size_t)(r - q0) * dim + i];
                treelik_rescale(o.data(), dim);
                if (c >= nleaves) std::copy(o.begin(), o.end(), O.begin() + (size_t)(c - nleaves) * dim);
                double A[3];
                for (int x = 0; x < 3; ++x) {
                    if (x == 0) std::copy(S.begin() + (size_t)(qq - q0) * dim, S.begin() + (size_t)(qq - q0 + 1) * dim, T.begin());
                    else treelik_apply(P + estride * c + mat * x, dim, partial(c), value(c), T.data());
                    double acc = 0.0;
                    for (uint32_t i = 0; i < dim; ++i) acc = acc + o[i] * T[i];
                    A[x] = acc;
                }
                g[c] = A[1] / A[0];
                q[c] = A[2] / A[0];
            }
        }
    }
    // After operator() on site s under the same P (P alone: derivs == false): the down pass with S from P, and per inner node v
    // a[(v - nleaves) * dim + i] = m(i) / Z with m(i) = B_v(i) U_v(i), Z = sum_i m(i) ascending; 0.0 where Z == 0.0
    void posteriors(uint32_t s, const double *P, double *a) {
        const uint32_t root = nnodes - 1;
        const size_t mat = (size_t)dim * dim;
        auto partial = [&](uint32_t c) -> const double * { return c < nleaves ? nullptr : &U[(size_t)(c - nleaves) * dim]; };
        auto value = [&](uint32_t c) -> int { return c < nleaves ? (int)rows[(size_t)c * ncols + s] : 0; };
        for (uint32_t v = root; v >= nleaves; --v) {
            if (v == root) for (uint32_t i = 0; i < dim; ++i) base[i] = pi[i];
            else {
                const double *Ov = &O[(size_t)(v - nleaves) * dim], *Pv = P + mat * v;
                for (uint32_t i = 0; i < dim; ++i) {
                    double acc = 0.0;
                    for (uint32_t h = 0; h < dim; ++h) acc = acc + Ov[h] * Pv[h + (size_t)dim * i];
                    base[i] = acc;
                }
            }
            if (a) {   // (null: the outside vectors alone, what tree_nni_host reads)
                const double *Uv = &U[(size_t)(v - nleaves) * dim];
                double *av = a + (size_t)(v - nleaves) * dim, Z = 0.0;
                for (uint32_t i = 0; i < dim; ++i) { av[i] = base[i] * Uv[i]; Z = Z + av[i]; }
                for (uint32_t i = 0; i < dim; ++i) av[i] = Z == 0.0 ? 0.0 : av[i] / Z;
            }
            const uint32_t q0 = ch.off[v], q1 = ch.off[v + 1];
            for (uint32_t qq = q0; qq < q1; ++qq) treelik_apply(P + mat * ch.idx[qq], dim, partial(ch.idx[qq]), value(ch.idx[qq]), &S[(size_t)(qq - q0) * dim]);
            for (uint32_t qq = q0; qq < q1; ++qq) {
                const uint32_t c = ch.idx[qq];
                if (c < nleaves) continue;   // (a leaf's outside vector has no reader)
                double *Oc = &O[(size_t)(c - nleaves) * dim];
                for (uint32_t i = 0; i < dim; ++i) Oc[i] = base[i];
                for (uint32_t r = q0; r < q1; ++r)
                    if (r != qq) for (uint32_t i = 0; i < dim; ++i) Oc[i] = Oc[i] * S[(size_t)(r - q0) * dim + i];
                treelik_rescale(Oc, dim);
            }
        }
    }
};
}  // namespace

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
