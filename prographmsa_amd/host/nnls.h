// nnls.h — NNLS (reference src/NNLS.h) for the weighted least-squares refinement of the guide tree (wls.cpp).
//
// The reference's active-set loop (TOL 1e-6, MAX_ITER 100) restated literally over small row-major matrices.  Its inner
// least-squares solves use Eigen's JacobiSVD (`Zp.jacobiSvd(ComputeThinU | ComputeThinV).solve(x)`), which is not available
// here; svd_solve below is a one-sided (Hestenes) Jacobi SVD instead.  Both give x = V diag(1 / s) U^T b over the singular
// values above the same threshold (min(rows, cols) * epsilon * the largest), i.e. the minimum-norm least-squares solution.
// They differ in how they get there: Eigen first reduces a tall matrix to a square R by a column-pivoting QR and then runs a
// two-sided Jacobi sweep on R; this orthogonalises the columns of the matrix itself.  On the full-rank 6 x 5 and 10 x 7
// systems of the refinement the two agree to rounding (a few units in the last place), not bit for bit.
// Header-only so that a test harness (tests/native/nnls_test.cpp) compiles the same code.
#ifndef PGM_NNLS_H_
#define PGM_NNLS_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace pgm {
namespace nnls {

// Least-squares solution of A x = b, A rows x cols row-major (rows >= cols), by a one-sided Jacobi SVD.
inline void svd_solve(int rows, int cols, const double *A, const double *b, double *x) {
    std::vector<double> U(A, A + (size_t)rows * cols), V((size_t)cols * cols, 0.0);
    for (int j = 0; j < cols; ++j) V[(size_t)j * cols + j] = 1.0;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < cols - 1; ++p)
            for (int q = p + 1; q < cols; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < rows; ++i) {
                    const double up = U[(size_t)i * cols + p], uq = U[(size_t)i * cols + q];
                    alpha += up * up;
                    beta += uq * uq;
                    gamma += up * uq;
                }
                if (gamma == 0 || std::fabs(gamma) <= eps * std::sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
                const double c = 1 / std::sqrt(1 + t * t), s = c * t;
                for (int i = 0; i < rows; ++i) {
                    double &up = U[(size_t)i * cols + p], &uq = U[(size_t)i * cols + q];
                    const double a = up, bq = uq;
                    up = c * a - s * bq;
                    uq = s * a + c * bq;
                }
                for (int i = 0; i < cols; ++i) {
                    double &vp = V[(size_t)i * cols + p], &vq = V[(size_t)i * cols + q];
                    const double a = vp, bq = vq;
                    vp = c * a - s * bq;
                    vq = s * a + c * bq;
                }
            }
        if (!rotated) break;
    }
    std::vector<double> sv(cols);
    double smax = 0;
    for (int j = 0; j < cols; ++j) {
        double s2 = 0;
        for (int i = 0; i < rows; ++i) s2 += U[(size_t)i * cols + j] * U[(size_t)i * cols + j];
        sv[j] = std::sqrt(s2);
        if (sv[j] > smax) smax = sv[j];
    }
    const double thr = std::max(smax * (double)std::min(rows, cols) * eps, std::numeric_limits<double>::min());
    for (int j = 0; j < cols; ++j) x[j] = 0;
    for (int j = 0; j < cols; ++j) {
        if (!(sv[j] > thr)) continue;
        double ub = 0;   // (U_j / s_j)^T b / s_j
        for (int i = 0; i < rows; ++i) ub += U[(size_t)i * cols + j] * b[i];
        ub /= sv[j] * sv[j];
        for (int i = 0; i < cols; ++i) x[i] += V[(size_t)i * cols + j] * ub;
    }
}

// NNLS.h:8-111: d >= 0 minimising |Z d - x|, Z rows x cols row-major (cols <= 16).  Returns the active-set iterations run
// (0: the unconstrained solution was already non-negative).
inline int solve(int rows, int cols, const double *Z, const double *x, double *d) {
    const double TOL = 1e-6;
    const int MAX_ITER = 100;
    svd_solve(rows, cols, Z, x, d);
    double dmin = d[0];
    for (int i = 1; i < cols; ++i) dmin = std::min(dmin, d[i]);
    if (dmin >= 0) return 0;

    bool P[16] = {};
    double w[16], dp[16], sp[16], alpha[16];
    int mapping[16];
    std::vector<double> Zp, r(rows);
    for (int i = 0; i < cols; ++i) d[i] = 0;
    auto gradient = [&]() {   // w = Z^T (x - Z d), zero on the passive set
        for (int i = 0; i < rows; ++i) {
            double zd = 0;
            for (int j = 0; j < cols; ++j) zd += Z[(size_t)i * cols + j] * d[j];
            r[i] = x[i] - zd;
        }
        for (int j = 0; j < cols; ++j) {
            double s = 0;
            for (int i = 0; i < rows; ++i) s += Z[(size_t)i * cols + j] * r[i];
            w[j] = s * (1.0 - (P[j] ? 1.0 : 0.0));
        }
    };
    gradient();
    int iiw = 0, n_iter = 0;
    auto all_p = [&]() { for (int i = 0; i < cols; ++i) if (!P[i]) return false; return true; };
    auto max_w = [&](int &iw) { iw = 0; for (int i = 1; i < cols; ++i) if (w[i] > w[iw]) iw = i; return w[iw]; };   // (first of equal maxima, as Eigen)
    int iw = 0;
    while (!all_p() && max_w(iw) > TOL) {
        P[iw] = true;
        if (n_iter++ > MAX_ITER) return n_iter;
        while (true) {
            int np = 0;
            for (int i = 0; i < cols; ++i)
                if (P[i]) {
                    dp[np] = d[i];
                    mapping[np] = i;
                    if (i == iw) iiw = np;
                    ++np;
                }
            Zp.resize((size_t)rows * np);   // the columns of the passive set
            for (int row = 0; row < rows; ++row)
                for (int k = 0; k < np; ++k) Zp[(size_t)row * np + k] = Z[(size_t)row * cols + mapping[k]];
            svd_solve(rows, np, Zp.data(), x, sp);
            double spmin = sp[0];
            for (int i = 1; i < np; ++i) spmin = std::min(spmin, sp[i]);
            if (spmin > 0) {
                for (int i = 0; i < np; ++i) d[mapping[i]] = sp[i];
                gradient();
                break;
            } else if (sp[iiw] <= 0) {
                w[iw] = 0;
                break;
            }
            for (int i = 0; i < np; ++i) alpha[i] = sp[i] > 0 ? INFINITY : dp[i] / (dp[i] - sp[i]);
            int ia = 0;
            for (int i = 1; i < np; ++i) if (alpha[i] < alpha[ia]) ia = i;   // (first of equal minima, as Eigen)
            const double a = alpha[ia];
            for (int i = 0; i < np; ++i) dp[i] = dp[i] + a * (sp[i] - dp[i]);
            for (int i = 0; i < np; ++i) {
                if (dp[i] <= 0 || i == ia) { P[mapping[i]] = false; d[mapping[i]] = 0; }
                else d[mapping[i]] = dp[i];
            }
        }
    }
    return n_iter;
}

}  // namespace nnls
}  // namespace pgm
#endif
