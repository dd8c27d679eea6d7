// treelik_nni.cpp — nearest-neighbour interchanges for `pgmsa --ml_tree --ml_search` (the walk and the checks are
// treelik_internal.h's): the host statement of pgm_tree_nni (Backend::tree_nni's
// default, what pgmsa_oracle runs), the gain of a candidate both drivers share, and the topology search, which is host code and the
// same for every backend.  For --ml_nni_opt: the host statement of pgm_tree_nni_edge and ml_nni_edge_lengths, the
// optimiser of every candidate's central branch, host code the search and ml_branch_support (treelik_support.cpp) share.
#include "treelik_internal.h"

#include <chrono>

namespace pgm {

MlSearchStats ml_search_stats;
MlNniOptStats ml_nni_opt_stats;
MlSprStats ml_spr_stats;   // (here, beside the search that counts its applied moves: host/treelik_spr.cpp is not linked by every program over the search)

namespace {
// tree_nni_host (Pc, d1, d2 null) and tree_nni_edge_host: one body, so the pieces both share are formed by the same lines
void tree_nni_body(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                   const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, const double *Pc,
                   double *site_l, int32_t *site_k, double *post, double *rho, double *d1, double *d2, size_t block_bytes) {
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
    std::vector<double> c1(Pc ? (size_t)ncand * nchunks : 0), c2(c1.size());   // the chunk sums of g and h, [candidate][chunk]
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
            double a1 = 0.0, a2 = 0.0;
            for (uint32_t s = s0; s < s1; ++s) {
                double mixed = 0.0, G = 0.0, Q = 0.0;
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
                    double A[2], A12[2] = {0.0, 0.0};   // (A12: the neighbour's sums under P' and P'', with Pc only)
                    int32_t count[2];
                    for (int side = 0; side < 2; ++side) {   // the tree as it is, then the neighbour
                        const double *Sx = side == 0 ? Sa.data() : Sc.data(), *Sy = side == 0 ? Sc.data() : Sa.data();
                        for (uint32_t i = 0; i < dim; ++i) { X[i] = T[i] * Sx[i]; Y[i] = R[i] * Sy[i]; }
                        count[side] = (treelik_rescale(X.data(), dim) ? 1 : 0) + (treelik_rescale(Y.data(), dim) ? 1 : 0);
                        const double *Z = side == 1 && Pc ? Pc + ((size_t)k * ncand + q) * 3 * mat : Pk + mat * v;   // the neighbour's own edge above v
                        treelik_apply(Z, dim, X.data(), 0, S.data());   // W
                        double acc = 0.0;
                        for (uint32_t i = 0; i < dim; ++i) acc = acc + Y[i] * S[i];
                        A[side] = acc;
                        for (int x = 1; side == 1 && Pc && x < 3; ++x) {
                            treelik_apply(Z + mat * x, dim, X.data(), 0, S.data());
                            acc = 0.0;
                            for (uint32_t i = 0; i < dim; ++i) acc = acc + Y[i] * S[i];
                            A12[x - 1] = acc;
                        }
                    }
                    double r = 0.0, r1 = 0.0, r2 = 0.0;
                    if (A[0] != 0.0) {
                        r = A[1] / A[0]; r1 = A12[0] / A[0]; r2 = A12[1] / A[0];
                        for (int32_t d = count[1] - count[0]; d > 0; --d) { r = r * kTreelikTiny; r1 = r1 * kTreelikTiny; r2 = r2 * kTreelikTiny; }
                        for (int32_t d = count[0] - count[1]; d > 0; --d) { r = r * kTreelikScale; r1 = r1 * kTreelikScale; r2 = r2 * kTreelikScale; }
                    }
                    const double pk = post[(size_t)k * ncols + s];
                    mixed = mixed + pk * r;
                    G = G + pk * r1;
                    Q = Q + pk * r2;
                }
                rho[(size_t)q * ncols + s] = mixed;
                if (Pc) {
                    double g = 0.0, h = 0.0;
                    if (mixed != 0.0) { g = G / mixed; h = Q / mixed - g * g; }
                    a1 = a1 + g;
                    a2 = a2 + h;
                }
            }
            if (Pc) { c1[(size_t)q * nchunks + chunk] = a1; c2[(size_t)q * nchunks + chunk] = a2; }
        });
    }
    for (uint32_t q = 0; Pc && q < ncand; ++q) {   // the chunk sums ascending
        double a1 = 0.0, a2 = 0.0;
        for (size_t chunk = 0; chunk < nchunks; ++chunk) { a1 = a1 + c1[(size_t)q * nchunks + chunk]; a2 = a2 + c2[(size_t)q * nchunks + chunk]; }
        d1[q] = a1;
        d2[q] = a2;
    }
}
}  // namespace

void tree_nni_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                   const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, double *site_l,
                   int32_t *site_k, double *post, double *rho, size_t block_bytes) {
    tree_nni_body(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cand_v, cand_a, cand_c, nullptr, site_l, site_k, post, rho, nullptr, nullptr, block_bytes);
}

void tree_nni_edge_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                        const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, const double *Pc,
                        double *site_l, int32_t *site_k, double *post, double *rho, double *d1, double *d2, size_t block_bytes) {
    if (!Pc || !d1 || !d2) error("tree likelihood: null argument");
    tree_nni_body(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cand_v, cand_a, cand_c, Pc, site_l, site_k, post, rho, d1, d2, block_bytes);
}

void Backend::tree_nni_edge(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                            const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, const double *Pc,
                            double *site_l, int32_t *site_k, double *post, double *rho, double *d1, double *d2, int) {
    tree_nni_edge_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, ncand, cand_v, cand_a, cand_c, Pc, site_l, site_k, post, rho, d1, d2);
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

MlNniEdgeResult ml_nni_edge_lengths(const ModelFactory &mf, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                    const std::vector<double> &rates, const double *P, const std::vector<double> &lengths, uint32_t ncand, const uint32_t *cand_v,
                                    const uint32_t *cand_a, const uint32_t *cand_c, uint32_t rounds, Backend *be, size_t pc_bytes) {
    const uint32_t ncat = rates.empty() ? 1u : (uint32_t)rates.size();
    const std::vector<double> r = rates.empty() ? std::vector<double>(1, 1.0) : rates;   // (one rate of 1.0: 1.0 * x is exact, the matrices are the plain ones)
    const std::vector<double> w(ncat, rates.empty() ? 1.0 : 1.0 / (double)ncat);
    return ml_nni_edge_lengths([&](const std::vector<double> &t, std::vector<double> &Pc) { treelik_matrices(mf, t, true, r, Pc); }, (uint32_t)mf.dim(), nleaves, nnodes, parent,
                               ncols, rows, mf.freqs().data(), ncat, w.data(), P, lengths, ncand, cand_v, cand_a, cand_c, rounds, be, pc_bytes);
}

MlNniEdgeResult ml_nni_edge_lengths(const MlNniEdgeMatrices &matrices, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols,
                                    const int8_t *rows, const double *pi, uint32_t ncat, const double *w, const double *P, const std::vector<double> &lengths, uint32_t ncand,
                                    const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, uint32_t rounds, Backend *be, size_t pc_bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!cand_v || ncand == 0) error("tree nni: no candidate");
    for (uint32_t q = 0; q < ncand; ++q)
        if (cand_v[q] >= lengths.size()) error("tree nni: candidate %u: v is not an inner node below the root", q);
    MlNniEdgeResult out;
    out.t_opt.resize(ncand); out.gain_opt.resize(ncand); out.rho.resize((size_t)ncand * ncols);
    out.site_l.resize(ncols); out.site_k.resize(ncols); out.post.resize((size_t)ncat * ncols);
    auto clamp = [](double x) { return x < kMlMinLength ? kMlMinLength : x > kMlMaxLength ? kMlMaxLength : x; };
    // the candidates in groups whose Pc stays within pc_bytes; every group is a call, which walks the tree again (the entries are stateless)
    const size_t per_call = std::max<size_t>(1, pc_bytes / (24 * (size_t)ncat * dim * dim));
    std::vector<double> best_d1(ncand), best_d2(ncand), lambda(ncand, 1.0), trial(ncand), d1(ncand), d2(ncand), gain(ncand), rho((size_t)ncand * ncols), Pc, tg;
    for (uint32_t round = 0; round <= rounds; ++round) {
        for (uint32_t q = 0; q < ncand; ++q) {
            if (round == 0) { trial[q] = lengths[cand_v[q]]; continue; }   // the tree's own length: rho is tree_nni's
            const double t = out.t_opt[q], target = best_d2[q] < 0 ? t - best_d1[q] / best_d2[q] : best_d1[q] > 0 ? 2 * t : t / 2;
            trial[q] = clamp(t + lambda[q] * (clamp(target) - t));
        }
        for (size_t q0 = 0; q0 < ncand; q0 += per_call) {
            const uint32_t g = (uint32_t)std::min<size_t>(per_call, ncand - q0);
            tg.assign(trial.begin() + q0, trial.begin() + q0 + g);
            matrices(tg, Pc);
            double *rh = rho.data() + q0 * ncols;
            if (be) be->tree_nni_edge(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, g, cand_v + q0, cand_a + q0, cand_c + q0, Pc.data(), out.site_l.data(),
                                      out.site_k.data(), out.post.data(), rh, d1.data() + q0, d2.data() + q0);
            else tree_nni_edge_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, g, cand_v + q0, cand_a + q0, cand_c + q0, Pc.data(), out.site_l.data(),
                                    out.site_k.data(), out.post.data(), rh, d1.data() + q0, d2.data() + q0);
            ++ml_nni_opt_stats.calls;
        }
        // the gains: candidates on the host threads, each sum in site order (treelik_nni_gain of the row)
        parallel_for(ncand, [&](size_t q) { treelik_nni_gain(1, ncols, rho.data() + q * ncols, &gain[q]); });
        for (uint32_t q = 0; q < ncand; ++q) {
            if (round == 0 || gain[q] > out.gain_opt[q]) {
                out.t_opt[q] = trial[q]; out.gain_opt[q] = gain[q]; best_d1[q] = d1[q]; best_d2[q] = d2[q]; lambda[q] = 1.0;
                std::copy(rho.begin() + (size_t)q * ncols, rho.begin() + (size_t)(q + 1) * ncols, out.rho.begin() + (size_t)q * ncols);
            } else lambda[q] = lambda[q] * 0.5;
        }
    }
    ml_nni_opt_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
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
                                  uint32_t search_rounds, uint32_t rounds, double eps, Backend *be, const MlGamma &gamma, uint32_t nni_opt, const MlSprHook *spr) {
    const auto t0 = std::chrono::steady_clock::now();
    MlSearchResult out;
    out.tree.reset(start.copy());
    out.res = ml_branch_lengths(a, rows, model_factory, *out.tree, rounds, eps, be, gamma);
    const double lnl_start = out.res.lnl_start;
    const uint32_t dim = (uint32_t)model_factory.dim(), ncols = (uint32_t)rows[0].size();
    std::vector<int8_t> flat;
    for (const auto &r : rows) flat.insert(flat.end(), r.begin(), r.end());
    const double *pi = model_factory.freqs().data();

    // one evaluation of `tree` without derivatives at the lengths it carries and the rates in hand (ml_tree_topology numbers it)
    auto lnl_of_tree = [&](const PhyTree &tree) -> double {
        const MlTreeTopology nt = ml_tree_topology(tree);
        const uint32_t ncat = out.res.rates.empty() ? 1u : (uint32_t)out.res.rates.size();
        const std::vector<double> w(ncat, out.res.rates.empty() ? 1.0 : 1.0 / (double)ncat);
        std::vector<double> P, site_l(ncols), post((size_t)ncat * ncols), t(nt.nnodes - 1);
        std::vector<int32_t> site_k(ncols);
        for (uint32_t e = 0; e + 1 < nt.nnodes; ++e) t[e] = nt.node[e]->getBranchLength();
        if (out.res.rates.empty()) {
            treelik_matrices(model_factory, t, false, P);
            if (be) be->tree_likelihood(dim, nt.nleaves, nt.nnodes, nt.parent.data(), ncols, flat.data(), pi, P.data(), 0, site_l.data(), site_k.data(), nullptr, nullptr);
            else tree_likelihood_host(dim, nt.nleaves, nt.nnodes, nt.parent.data(), ncols, flat.data(), pi, P.data(), 0, site_l.data(), site_k.data(), nullptr, nullptr);
        } else {
            treelik_matrices(model_factory, t, false, out.res.rates, P);
            if (be) be->tree_likelihood_rates(dim, nt.nleaves, nt.nnodes, nt.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), 0, site_l.data(), site_k.data(),
                                              post.data(), nullptr, nullptr);
            else tree_likelihood_rates_host(dim, nt.nleaves, nt.nnodes, nt.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), 0, site_l.data(), site_k.data(),
                                            post.data(), nullptr, nullptr);
        }
        ++ml_tree_stats.evaluations;
        return treelik_lnl(ncols, site_l.data(), site_k.data(), nullptr);
    };
    // a moved tree that raised lnL becomes the search's: ml_branch_lengths from the carried lengths and the shape in hand
    auto accept = [&](std::unique_ptr<PhyTree> tree) {
        MlGamma from = gamma;
        if (gamma.ncat >= 2 && gamma.estimate) from.start = out.res.alpha;
        out.tree = std::move(tree);
        out.res = ml_branch_lengths(a, rows, model_factory, *out.tree, rounds, eps, be, from);
    };
    // --ml_spr: the scan of a round whose interchanges applied no move; true: a move was applied
    auto spr_step = [&](uint32_t round) -> bool {
        const MlTreeTopology topo = ml_tree_topology(*out.tree);
        const MlSprScan scan = spr->scan(model_factory, topo, out.res, ncols, flat.data(), spr->radius, eps, be, kSprRhoBytes);
        MlSearchRound line;
        line.round = round; line.spr = true; line.candidates = scan.candidates; line.positive = scan.positive; line.best_gain = scan.best_gain;
        line.lnl_before = line.lnl_applied = line.lnl_after = out.res.lnl;
        bool accepted = false;
        for (size_t m = scan.pick_v.size(); m >= 1 && !accepted; m = m / 2) {
            std::unique_ptr<PhyTree> tree(spr->apply(topo, out.res.lengths, (uint32_t)m, scan.pick_v.data(), scan.pick_y.data()));
            const double there = lnl_of_tree(*tree);
            if (there > line.lnl_before) {
                accepted = true;
                line.applied = (uint32_t)m;
                line.lnl_applied = there;
                accept(std::move(tree));
                line.lnl_after = out.res.lnl;
            }
        }
        out.log.push_back(line);
        if (!accepted) return false;
        ++ml_search_stats.rounds;
        ml_spr_stats.applied += line.applied;
        return true;
    };

    // the interchange step of a round; true: a move was applied
    auto nni_step = [&](uint32_t round) -> bool {
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
        if (cv.empty()) { out.log.push_back(line); return false; }   // (a tree whose root alone is an inner node)
        const uint32_t ncand = (uint32_t)cv.size();
        const uint32_t ncat = out.res.rates.empty() ? 1u : (uint32_t)out.res.rates.size();
        const std::vector<double> w(ncat, out.res.rates.empty() ? 1.0 : 1.0 / (double)ncat);
        std::vector<double> P, site_l(ncols), post((size_t)ncat * ncols), rho(nni_opt ? 0 : (size_t)ncand * ncols), gain(ncand);
        std::vector<int32_t> site_k(ncols);
        if (out.res.rates.empty()) treelik_matrices(model_factory, out.res.lengths, false, P);
        else treelik_matrices(model_factory, out.res.lengths, false, out.res.rates, P);
        std::vector<double> t_opt;   // with nni_opt: the central length every candidate is ranked at
        if (nni_opt) {
            MlNniEdgeResult opt = ml_nni_edge_lengths(model_factory, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), out.res.rates, P.data(), out.res.lengths, ncand, cv.data(),
                                                      ca.data(), cc.data(), nni_opt, be);
            gain.swap(opt.gain_opt);
            t_opt.swap(opt.t_opt);
        } else {
            if (be) be->tree_nni(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), ncand, cv.data(), ca.data(), cc.data(), site_l.data(),
                                 site_k.data(), post.data(), rho.data());
            else tree_nni_host(dim, nleaves, nnodes, topo.parent.data(), ncols, flat.data(), pi, ncat, w.data(), P.data(), ncand, cv.data(), ca.data(), cc.data(), site_l.data(),
                               site_k.data(), post.data(), rho.data());
            treelik_nni_gain(ncand, ncols, rho.data(), gain.data());
        }
        ++ml_search_stats.calls;
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
        if (picked.empty()) { out.log.push_back(line); return false; }
        bool accepted = false;
        for (size_t m = picked.size(); m >= 1 && !accepted; m = m / 2) {
            MlSearchTree next = cur;
            for (size_t p = 0; p < m; ++p) {   // a and c exchanged: both keep their length, each takes the other's place among the children
                const uint32_t q = picked[p], v = cv[q], u = topo.parent[v];
                *std::find(next.kids[v].begin(), next.kids[v].end(), ca[q]) = cc[q];
                *std::find(next.kids[u].begin(), next.kids[u].end(), cc[q]) = ca[q];
                if (nni_opt) next.length[v] = t_opt[q];   // the length the move was ranked at
            }
            std::unique_ptr<PhyTree> tree(ml_search_build(next, next.root));
            const double there = lnl_of_tree(*tree);
            if (there > line.lnl_before) {
                accepted = true;
                line.applied = (uint32_t)m;
                line.lnl_applied = there;
                accept(std::move(tree));
                line.lnl_after = out.res.lnl;
            }
        }
        out.log.push_back(line);
        if (!accepted) return false;
        ++ml_search_stats.rounds;
        ml_search_stats.applied += line.applied;
        return true;
    };

    for (uint32_t round = 1; round <= search_rounds; ++round) {
        if (nni_step(round)) continue;
        if (!spr || !spr_step(round)) break;   // (the search ends where no step applies a move)
    }
    out.res.lnl_start = lnl_start;
    ml_tree_stats.lnl_start = lnl_start;
    ml_search_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
}

}  // namespace pgm
