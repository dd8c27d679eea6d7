// treelik.h — the declarations of the --ml_* analyses (host/treelik*.cpp); pgm_host.h includes it, so nobody else has to.
#pragma once
#include "pgm_host.h"

#include <functional>

namespace pgm {

// --ml_tree: the likelihood of an alignment on a rooted tree and maximum-likelihood branch lengths on its fixed topology
// (host/treelik.cpp).
// tree_likelihood_host: pgm_tree_likelihood (include/pgm_hip.h) by a loop over the sites on the host threads, the same contract and
//   the same bits; what it rejects is an error().  Backend::tree_likelihood's default.
// MlTreeTopology: the nodes of a tree numbered children before parents, the leaves first in sorted-name order, the inner nodes in
//   post-order, the root last; edge e is the edge above node e.
// treelik_matrices: P(t_e), Q P(t_e), Q Q P(t_e) of every edge back to back (derivs) or P(t_e) alone, as pgm_tree_likelihood reads them.
// treelik_lnl: sum over the sites of log(site_l) - 256 ln 2 site_k, sites ascending; site_lnl (may be null) gets the terms.
// ml_branch_lengths: the optimiser.  rows: the alignment's rows in sorted-name order as state values (0..dim-1, -1 a gap, -2 a residue
//   without a value), all of one length.  be: the backend whose tree_likelihood runs, nullptr for the host loop.
// --ml_gamma (host/treelik_rates.cpp):
// tree_likelihood_rates_host: pgm_tree_likelihood_rates by the same loop, Backend::tree_likelihood_rates's default.
// gamma_rates: the K rates of the discrete gamma of shape alpha (Yang 1994, category means), equally probable, their mean 1.
// treelik_matrices with rates: category-major, for category c and edge e P(r_c t_e), r_c Q P, r_c^2 Q Q P.
// MlGamma: what ml_branch_lengths is asked for (ncat < 2: one rate for every column, the loop of --ml_tree alone); with `estimate`
//   alpha starts at 1 and the branch-length loop alternates with a golden-section search on ln alpha.
// --ml_ancestral (host/treelik_anc.cpp):
// tree_ancestral_host: pgm_tree_ancestral by the same loop, Backend::tree_ancestral's default.
// tree_ancestral_presence: the gap rule of the written records, present[(v - nleaves) * ncols + s] = 1 iff inner node v lies on a
//   path between two leaves whose row at column s is not -1 (parent: the numbering of the likelihood entries).
// --ml_search (host/treelik_nni.cpp):
// tree_nni_host: pgm_tree_nni per block of column chunks (the walk's partials and outside vectors of a block are held, 256 MB by
//   default) by a loop over the block's columns, then over candidates x column chunks; Backend::tree_nni's default.
// treelik_nni_gain: gain[q] = sum over the sites ascending of log rho[q][s] (log 0 is -infinity).
// ml_topology_search: ml_branch_lengths on the start tree, then up to `search_rounds` rounds of: one tree_nni call over every
//   candidate (v ascending, a in child order, c in child order), the candidates of gain > eps by gain descending then index, picked
//   greedily while no two share a node of {u, v, a, c}; the first m picked applied (m from all of them, halved while the evaluation at
//   the carried lengths is not above lnL; none left: the search ends), then ml_branch_lengths again from the carried lengths and
//   the shape in hand.  lnL never decreases.  With nni_opt the candidates are ranked by ml_nni_edge_lengths's gain_opt and an applied
//   move gives the edge above v its t_opt.  With `spr` (--ml_spr) a round whose interchange step applies no move, where
//   the search would end, logs that step and runs an SPR scan (ml_spr_scan): its picks go through the same acceptance (the first m
//   applied, one evaluation, halved while lnL does not rise), an accepted scan is a round and the search goes on; the search ends
//   where the scan applies no move either.
const double kMlMinLength = 1e-6, kMlMaxLength = 10.0;   // the interval every branch length stays in
const double kMlMinAlpha = 0.05, kMlMaxAlpha = 100.0;     // ... and the shape of the gamma
const uint32_t kMlAlphaEvaluations = 12, kMlMaxPairs = 20;   // one search on ln alpha; branch-length loop + search pairs at the most
// alignments of this many taxa and more go to the device by default: the smallest size at which the two routes were timed, and the
// device was faster there and at every larger one (measured once); below it the host loop runs, untimed
const uint32_t kTreelikDeviceMin = 24;
struct MlTreeStats {   // `pgmsa --ml_tree --stats`
    double seconds = 0, kernel_ms = 0, lnl_start = 0, lnl = 0;
    double ancestral_s = 0;    // --ml_ancestral only: the tree_ancestral call, its matrices included
    double ancestral_joint_s = 0, ancestral_samples_s = 0;   // --ml_ancestral_joint, --ml_ancestral_samples only: the same of their calls
    uint64_t rounds = 0, evaluations = 0;
    uint32_t categories = 0;   // --ml_gamma only
    double alpha = 0;
};
extern MlTreeStats ml_tree_stats;
struct MlTreeTopology {
    uint32_t nleaves = 0, nnodes = 0;
    std::vector<uint32_t> parent;           // nnodes, the root's: UINT32_MAX
    std::vector<const PhyTree *> node;      // nnodes
    std::vector<std::string> names;         // the leaves' names, sorted
};
MlTreeTopology ml_tree_topology(const PhyTree &tree);
void tree_likelihood_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                          const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2);
void treelik_matrices(const ModelFactory &mf, const std::vector<double> &t /* nnodes - 1 */, bool derivs, std::vector<double> &P);
double treelik_lnl(uint32_t ncols, const double *site_l, const int32_t *site_k, double *site_lnl);
void tree_likelihood_rates_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post, double *d1, double *d2);
void tree_ancestral_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                         const double *w, const double *P, double *site_l, int32_t *site_k, double *post, int8_t *anc_state /* ninner x ncols */,
                         double *anc_prob /* ninner x ncols */, double *anc_post /* ninner x ncols x dim, or null */);
void tree_ancestral_presence(uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, uint8_t *present /* ninner x ncols */);
// --ml_ancestral_joint, --ml_ancestral_samples (host/treelik_joint.cpp):
// tree_ancestral_joint_host: pgm_tree_ancestral_joint by the same loop over the sites, Backend::tree_ancestral_joint's default.
// tree_ancestral_sample_host: pgm_tree_ancestral_sample by the same loop, the samples of a site inside; Backend::tree_ancestral_sample's
//   default.  A caller cuts its samples into calls whose samp_state stays within kSampleStateBytes (first_sample: the draws do not
//   depend on the cut).
void tree_ancestral_joint_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                               const double *w, const double *P, double *site_l, int32_t *site_k, double *post, uint8_t *cat /* ncols */,
                               int8_t *joint_state /* ninner x ncols */, double *joint_l /* ncols */, int32_t *joint_k /* ncols */);
void tree_ancestral_sample_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                                const double *w, const double *P, uint32_t nsamp, uint64_t first_sample, uint64_t seed, double *site_l, int32_t *site_k, double *post,
                                uint8_t *samp_cat /* ncols x nsamp */, int8_t *samp_state /* ninner x ncols x nsamp */);
std::vector<double> gamma_rates(double alpha, uint32_t K);
void treelik_matrices(const ModelFactory &mf, const std::vector<double> &t, bool derivs, const std::vector<double> &rates, std::vector<double> &P);
struct MlGamma {
    uint32_t ncat = 0;
    bool estimate = true;
    double alpha = 1.0;
    double start = 1.0;   // with `estimate`: the shape the search starts from
};
struct MlTreeResult {
    std::vector<double> lengths;    // per edge (node below it)
    std::vector<double> site_lnl;   // per column, at `lengths`
    double lnl_start = 0, lnl = 0;
    uint32_t rounds = 0, evaluations = 0;
    double alpha = 0;               // --ml_gamma only: the shape, the categories' rates, post (ncat x ncols) at `lengths`
    std::vector<double> rates, post;
};
MlTreeResult ml_branch_lengths(const Alphabet &a, const std::vector<std::vector<int8_t>> &rows, const ModelFactory &model_factory, const PhyTree &tree,
                               uint32_t rounds, double eps, Backend *be = nullptr, const MlGamma &gamma = MlGamma());
const size_t kTreelikNniBlockBytes = (size_t)256 << 20;
void tree_nni_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                   const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c /* ncand each */,
                   double *site_l, int32_t *site_k, double *post, double *rho /* ncand x ncols */,
                   size_t block_bytes = kTreelikNniBlockBytes /* the partials and outside vectors held at a time, about; at least one column chunk */);
void treelik_nni_gain(uint32_t ncand, uint32_t ncols, const double *rho, double *gain /* ncand */);
// --ml_nni_opt (host/treelik_nni.cpp):
// tree_nni_edge_host: pgm_tree_nni_edge blocked as tree_nni_host, the same contract and bits; Backend::tree_nni_edge's default.
// ml_nni_edge_lengths: the central branch of every candidate re-optimised, every candidate at once.  Round 0 evaluates every candidate
//   at the tree's own length of the edge above v (rho is tree_nni's bit for bit); rounds 1 .. `rounds` a trial
//   clamp(t_best + lambda (clamp(target) - t_best)), target = d2 < 0 ? t - d1 / d2 : d1 > 0 ? 2 t : t / 2 from the derivatives at t_best
//   (ml_branch_lengths's rule, the clamp to kMlMinLength .. kMlMaxLength).  A trial whose gain (treelik_nni_gain of its row) is higher
//   becomes the best, takes its derivatives, keeps its rho row and sets lambda to 1; otherwise lambda halves.  So gain_opt[q] is never
//   below the gain at the tree's own length.  rates: empty for one rate; P, lengths: the tree's matrices (P alone) and lengths.  The
//   candidates go in groups whose Pc stays within pc_bytes, one tree_nni_edge call per group and round.
const size_t kNniEdgeBytes = (size_t)256 << 20;   // Pc of one tree_nni_edge call
void tree_nni_edge_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                        const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c,
                        const double *Pc /* ncat x ncand x 3 x dim x dim */, double *site_l, int32_t *site_k, double *post, double *rho /* ncand x ncols */,
                        double *d1, double *d2 /* ncand each */, size_t block_bytes = kTreelikNniBlockBytes);
struct MlNniOptStats {   // `--ml_nni_opt --stats`
    double seconds = 0, kernel_ms = 0;
    uint64_t calls = 0;   // tree_nni_edge calls
};
extern MlNniOptStats ml_nni_opt_stats;
struct MlNniEdgeResult {
    std::vector<double> t_opt, gain_opt, rho;   // ncand; ncand; ncand x ncols, the rows at t_opt
    std::vector<double> site_l, post;           // the tree's own, as tree_nni gives them
    std::vector<int32_t> site_k;
};
MlNniEdgeResult ml_nni_edge_lengths(const ModelFactory &mf, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                    const std::vector<double> &rates, const double *P /* ncat x (nnodes-1) x dim x dim */, const std::vector<double> &lengths /* nnodes - 1 */,
                                    uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, uint32_t rounds, Backend *be = nullptr,
                                    size_t pc_bytes = kNniEdgeBytes);
// ... and with the matrices of the trial lengths from the caller: matrices(t, Pc) writes Pc (ncat x t.size() x 3 x dim x dim) for the
// candidates' lengths t, as treelik_matrices(mf, t, true, rates, Pc) does above
typedef std::function<void(const std::vector<double> &t, std::vector<double> &Pc)> MlNniEdgeMatrices;
MlNniEdgeResult ml_nni_edge_lengths(const MlNniEdgeMatrices &matrices, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols,
                                    const int8_t *rows, const double *pi, uint32_t ncat, const double *w, const double *P, const std::vector<double> &lengths, uint32_t ncand,
                                    const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, uint32_t rounds, Backend *be = nullptr,
                                    size_t pc_bytes = kNniEdgeBytes);
struct MlSearchStats {   // `pgmsa --ml_tree --ml_search --stats`
    double seconds = 0, kernel_ms = 0;
    uint64_t rounds = 0, applied = 0, calls = 0;   // accepted rounds, moves applied in them, tree_nni calls
};
extern MlSearchStats ml_search_stats;
struct MlSearchRound {   // a line of --ml_search_log
    uint32_t round = 0, candidates = 0, positive = 0, applied = 0;
    double best_gain = 0, lnl_before = 0, lnl_applied = 0, lnl_after = 0;
    bool spr = false;   // --ml_spr: the line of an SPR scan (the ninth column)
};
struct MlSprHook;   // (--ml_spr, below)
struct MlSearchResult {
    std::unique_ptr<PhyTree> tree;   // the searched tree; `res` is ml_branch_lengths's result on it (lnl_start: the start tree's)
    MlTreeResult res;
    std::vector<MlSearchRound> log;
};
MlSearchResult ml_topology_search(const Alphabet &a, const std::vector<std::vector<int8_t>> &rows, const ModelFactory &model_factory, const PhyTree &start,
                                  uint32_t search_rounds, uint32_t rounds, double eps, Backend *be = nullptr, const MlGamma &gamma = MlGamma(),
                                  uint32_t nni_opt = 0 /* --ml_nni_opt: the Newton rounds of ml_nni_edge_lengths, 0: rank at the lengths in hand */,
                                  const MlSprHook *spr = nullptr /* --ml_spr: a round whose interchanges apply no move runs an SPR scan */);
// --ml_spr (host/treelik_spr.cpp):
// tree_spr_host: pgm_tree_spr blocked as tree_nni_host, the same contract and bits, the candidates as a parallel_for over prune nodes x
//   column chunks; Backend::tree_spr's default.
// ml_spr_candidates: every valid candidate (v, y) of pgm_tree_spr whose path has at most `radius` edges, v ascending, then y ascending.
// ml_spr_touched: the nodes a move reads or changes: v, p, parent[p], the children of p, every node of the path, y and parent[y].
const size_t kSprRhoBytes = (size_t)256 << 20;   // rho of one tree_spr call
const size_t kSampleStateBytes = (size_t)256 << 20;   // samp_state of one tree_ancestral_sample call
void tree_spr_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                   const double *w, const double *P, const double *Ph /* as P: half of every edge */, uint32_t ncand, const uint32_t *cand_v,
                   const uint32_t *cand_y /* ncand each */, double *site_l, int32_t *site_k, double *post, double *rho /* ncand x ncols */,
                   size_t block_bytes = kTreelikNniBlockBytes);
void ml_spr_candidates(uint32_t nnodes, const uint32_t *parent, uint32_t radius, std::vector<uint32_t> &cand_v, std::vector<uint32_t> &cand_y);
std::vector<uint32_t> ml_spr_touched(uint32_t nnodes, const uint32_t *parent, uint32_t v, uint32_t y);
// ml_spr_apply: the tree after the first m of the given moves, whose touched sets are disjoint (lengths: per edge of topo): v keeps
//   t_v, y and the new node both get max(t_y / 2, kMlMinLength), a dissolved p gives its sibling min(t_p + t_s, kMlMaxLength).
// ml_spr_scan: every candidate within the radius scored at the lengths and rates of `res` (P and Ph from treelik_matrices, the half
//   lengths max(t_y / 2, kMlMinLength)), in groups of whole prune nodes whose rho stays within rho_bytes, one tree_spr call per group
//   (be: the backend, nullptr for the host loop); the gain of a candidate is treelik_nni_gain of its rho row; the candidates of
//   gain > eps by gain descending, then by index, picked greedily while their touched sets are disjoint.
struct MlSprScan {
    uint32_t candidates = 0, positive = 0;
    double best_gain = 0;
    std::vector<uint32_t> pick_v, pick_y;   // the picked moves in the order they were picked
};
PhyTree *ml_spr_apply(const MlTreeTopology &topo, const std::vector<double> &lengths, uint32_t m, const uint32_t *move_v, const uint32_t *move_y);
MlSprScan ml_spr_scan(const ModelFactory &mf, const MlTreeTopology &topo, const MlTreeResult &res, uint32_t ncols, const int8_t *rows, uint32_t radius, double eps,
                      Backend *be = nullptr, size_t rho_bytes = kSprRhoBytes);
// what ml_topology_search needs of the above (the driver fills it with ml_spr_scan and ml_spr_apply, so that the search itself and
// the stand-alone programs over it link without host/treelik_spr.cpp)
struct MlSprHook {
    uint32_t radius = 0;
    MlSprScan (*scan)(const ModelFactory &, const MlTreeTopology &, const MlTreeResult &, uint32_t, const int8_t *, uint32_t, double, Backend *, size_t) = nullptr;
    PhyTree *(*apply)(const MlTreeTopology &, const std::vector<double> &, uint32_t, const uint32_t *, const uint32_t *) = nullptr;
};
struct MlSprStats {   // `--ml_spr --stats`
    double seconds = 0, kernel_ms = 0;
    uint64_t calls = 0, candidates = 0, applied = 0;   // tree_spr calls, candidates scored, moves applied in accepted rounds
};
extern MlSprStats ml_spr_stats;
// --ml_support (host/treelik_support.cpp):
// resampled_sums_host: pgm_resampled_sums by a loop over rows x chunks of replicates on the host threads, the same contract and the
//   same bits; what it rejects is an error().  Backend::resampled_sums's default.
// ml_support_candidates: the supported nodes (every inner node v below the root whose parent is not a root of exactly two children),
//   ascending, and their candidates (v, a, c), a in child order, then c in child order: the other resolutions around the edge above v.
// ml_branch_support: one tree_nni call over those candidates, x = log rho, the observed gains (treelik_nni_gain), the resampled gains
//   D[q][r] by resampled_sums in groups of rows whose x stays within x_bytes, and per node with the candidates C whose gain is not
//   -infinity: d_obs = -max gain, alrt = 2 d_obs, sh_hits = the replicates whose largest of {0, D[q][r] - mean_q} is less than d_obs
//   ahead of the second largest (0 when d_obs <= 0), rell_hits = the replicates with D[q][r] <= 0 for every q of C; C empty:
//   alrt = +infinity and both counts nrep.  be: the backend whose tree_nni and resampled_sums run, nullptr for the host loops.
const size_t kSupportBytes = (size_t)1 << 30;   // x of one resampled_sums call
struct MlSupportStats {   // `pgmsa --ml_tree --ml_support --stats`
    double seconds = 0, kernel_ms = 0;
    uint64_t nodes = 0, calls = 0;   // supported nodes, resampled_sums calls
};
extern MlSupportStats ml_support_stats;
struct MlSupportNode {
    uint32_t node = 0, candidates = 0;   // the node's number, the candidates around the edge above it
    double alrt = 0;
    uint32_t sh_hits = 0, rell_hits = 0;
};
struct MlSupportOpt {   // --ml_nni_opt for ml_branch_support: x = log of ml_nni_edge_lengths's rho rows at t_opt
    uint32_t rounds = 0;
    const ModelFactory *mf = nullptr;
    const std::vector<double> *rates = nullptr, *lengths = nullptr;   // the categories' rates (empty: one rate), the tree's lengths
};
void resampled_sums_host(uint32_t nrow, uint32_t ncols, const double *x /* nrow x ncols */, uint32_t nrep, const uint32_t *cols /* nrep x ncols */,
                         double *out /* nrow x nrep */);
void ml_support_candidates(uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, std::vector<uint32_t> &node, std::vector<uint32_t> &cand_v,
                           std::vector<uint32_t> &cand_a, std::vector<uint32_t> &cand_c);
std::vector<MlSupportNode> ml_branch_support(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                             uint32_t ncat, const double *w, const double *P /* ncat x (nnodes-1) x dim x dim */, uint32_t nrep,
                                             const uint32_t *cols /* nrep x ncols */, Backend *be = nullptr, size_t x_bytes = kSupportBytes,
                                             const MlSupportOpt *opt = nullptr);
// a copy of `tree` whose edge above topo.node[e] has length lengths[e]
PhyTree *ml_tree_with_lengths(const MlTreeTopology &topo, const std::vector<double> &lengths);

}  // namespace pgm
