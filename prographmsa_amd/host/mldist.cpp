// mldist.cpp — the ML distance estimator and the scores of the all-pairs alignment
// (reference src/DistanceFactoryML.{h,cpp}, DistanceFactoryAlign.cpp).
// computeDistance of one pair from its count matrix on the host: Newton on d, each step a P(d) (estimate_distances in distance.cpp
// deals the pairs to the host threads, or sends them to pgm_mldist_batch, which keeps this operation order), and the limits of the
// estimate per alphabet; DistanceFactoryAlign's constructor reads the scoring matrix and gap costs of alignPair.
#include "pgm_host.h"
#include <algorithm>
#include <cmath>
#include <fstream>

namespace pgm {
// ---- DistanceFactoryML ---------------------------------------------------------------------
void mldist_limits(const Alphabet &a, double &DIST_MAX, double &VAR_MAX, double &VAR_MIN) {  // DistanceFactoryML.cpp:5-32
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
    mldist_limits(alphabet, DIST_MAX, VAR_MAX, VAR_MIN);
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
    mldist_limits(alphabet, DIST_MAX, VAR_MAX, VAR_MIN);
    double ident = 0, total = 0;
    for (int i = 0; i < n; ++i) ident += counts[i + n * i];
    for (int32_t c : counts) total += c;
    return computeDistance(ident, total, &counts, gaps, seqlen);
}

// (ident, total) are sums of integers, exact in any order: the all-pairs stage reduces them on the device when nothing else of the
// count matrix is read (no --mldist: counts == nullptr)
distvar_t DistanceFactoryML::computeDistance(double ident, double total, const std::vector<int32_t> *counts, index_t gaps, double seqlen) const {
    double DIST_MAX, VAR_MAX, VAR_MIN;
    mldist_limits(alphabet, DIST_MAX, VAR_MAX, VAR_MIN);
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
}  // namespace pgm
