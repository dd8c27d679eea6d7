// treelik_rates.cpp — rate variation across sites for `pgmsa --ml_tree --ml_gamma` (the walk is treelik_internal.h's;
// DESIGN.md 3.18): the host statement of pgm_tree_likelihood_rates (Backend::tree_likelihood_rates's default,
// what pgmsa_oracle runs), the rates of the discrete gamma, and the rate-folded matrices of every category and edge.
#include "treelik_internal.h"

namespace pgm {

void tree_likelihood_rates_host(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post, double *d1, double *d2) {
    if (!w || !post) error("tree likelihood: null argument");
    treelik_check_rates_host(ncat, w);
    const TreelikChildren ch = treelik_check_host(dim, nleaves, nnodes, parent, ncols, rows, pi, P, derivs, site_l, site_k, d1, d2);
    const uint32_t nedges = nnodes - 1;
    const size_t nchunks = ((size_t)ncols + kTreelikChunk - 1) / kTreelikChunk, pstride = (size_t)dim * dim * (derivs ? 3 : 1) * nedges;
    std::vector<double> c1, c2;   // per chunk and edge: the sums of g and h over the chunk's sites, ascending
    if (derivs) { c1.assign(nchunks * nedges, 0.0); c2.assign(nchunks * nedges, 0.0); }

    parallel_for(nchunks, [&](size_t chunk) {
        TreelikSiteWalk walk(ch, dim, nleaves, nnodes, ncols, rows, pi, derivs != 0);
        std::vector<double> gc((size_t)ncat * nedges), qc((size_t)ncat * nedges), L(ncat), term(ncat);
        std::vector<int32_t> k(ncat);
        const uint32_t s0 = (uint32_t)(chunk * kTreelikChunk), s1 = (uint32_t)std::min<size_t>(ncols, (size_t)s0 + kTreelikChunk);
        for (uint32_t s = s0; s < s1; ++s) {
            for (uint32_t c = 0; c < ncat; ++c) walk(s, P + pstride * c, L[c], k[c], &gc[(size_t)c * nedges], &qc[(size_t)c * nedges]);
            int32_t kmin = k[0];
            for (uint32_t c = 1; c < ncat; ++c) kmin = k[c] < kmin ? k[c] : kmin;
            double total = 0.0;
            for (uint32_t c = 0; c < ncat; ++c) {
                double t = w[c] * L[c];
                for (int32_t d = k[c] - kmin; d > 0; --d) t = t * kTreelikTiny;
                term[c] = t;
                total = total + t;
            }
            site_l[s] = total;
            site_k[s] = kmin;
            for (uint32_t c = 0; c < ncat; ++c) { term[c] = term[c] / total; post[(size_t)c * ncols + s] = term[c]; }
            if (!derivs) continue;
            for (uint32_t e = 0; e < nedges; ++e) {
                double g = 0.0, q = 0.0;
                for (uint32_t c = 0; c < ncat; ++c) {
                    g = g + term[c] * gc[(size_t)c * nedges + e];
                    q = q + term[c] * qc[(size_t)c * nedges + e];
                }
                c1[chunk * nedges + e] = c1[chunk * nedges + e] + g;
                c2[chunk * nedges + e] = c2[chunk * nedges + e] + (q - g * g);
            }
        }
    });
    if (!derivs) return;
    treelik_chunk_totals(c1, c2, nchunks, nedges, d1, d2);
}

void Backend::tree_likelihood_rates(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                    uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post, double *d1, double *d2,
                                    int) {
    tree_likelihood_rates_host(dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, derivs, site_l, site_k, post, d1, d2);
}

namespace {
// I(a, x): the regularised lower incomplete gamma function, by its series below x < a + 1 and by the continued fraction of the
// upper function (modified Lentz) from there on; both run until a term no longer changes the sum.
double gamma_lower_regularised(double a, double x) {
    if (!(x > 0.0)) return 0.0;
    if (x == INFINITY) return 1.0;
    const double front = std::exp(-x + a * std::log(x) - std::lgamma(a));
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int n = 0; n < 100000; ++n) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (std::fabs(del) <= std::fabs(sum) * 1e-17) break;
        }
        return sum * front;
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int n = 1; n < 100000; ++n) {
        const double an = -(double)n * ((double)n - a);
        b += 2.0;
        d = an * d + b; if (std::fabs(d) < tiny) d = tiny;
        c = b + an / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) <= 1e-17) break;
    }
    return 1.0 - front * h;
}
// y with I(a, y) = p, 0 < p < 1: bisection until the interval holds no further double
double gamma_quantile(double a, double p) {
    double lo = 0.0, hi = 1.0;
    while (gamma_lower_regularised(a, hi) < p) { lo = hi; hi *= 2.0; }
    for (;;) {
        const double mid = lo + (hi - lo) / 2;
        if (!(mid > lo && mid < hi)) return hi - mid < mid - lo ? hi : mid;
        if (gamma_lower_regularised(a, mid) < p) lo = mid; else hi = mid;
    }
}
}  // namespace

std::vector<double> gamma_rates(double alpha, uint32_t K) {
    if (!(alpha > 0.0 && alpha < INFINITY) || K < 1) error("gamma rates: shape %g, %u categories", alpha, K);
    std::vector<double> r(K);
    double below = 0.0;   // I(alpha + 1, alpha c_{k-1})
    for (uint32_t k = 1; k <= K; ++k) {
        const double here = k == K ? 1.0 : gamma_lower_regularised(alpha + 1.0, gamma_quantile(alpha, (double)k / (double)K));   // (alpha c_k: the quantile of scale 1)
        r[k - 1] = (double)K * (here - below);
        below = here;
    }
    double sum = 0.0;
    for (uint32_t k = 0; k < K; ++k) sum = sum + r[k];
    const double mean = sum / (double)K;
    for (uint32_t k = 0; k < K; ++k) r[k] = r[k] / mean;
    return r;
}

void treelik_matrices(const ModelFactory &mf, const std::vector<double> &t, bool derivs, const std::vector<double> &rates, std::vector<double> &P) {
    const size_t n = (size_t)mf.dim(), mat = n * n, stride = derivs ? 3 * mat : mat, nedges = t.size();
    std::vector<double> scaled(nedges), one;
    P.resize(stride * nedges * rates.size());
    for (size_t c = 0; c < rates.size(); ++c) {
        const double r = rates[c], rr = r * r;
        for (size_t e = 0; e < nedges; ++e) scaled[e] = r * t[e];
        treelik_matrices(mf, scaled, derivs, one);   // P(r t), Q P, Q Q P
        double *Pc = &P[stride * nedges * c];
        for (size_t e = 0; e < nedges; ++e)
            for (size_t x = 0; x < (derivs ? 3u : 1u); ++x) {
                const double f = x == 0 ? 1.0 : x == 1 ? r : rr;
                const double *src = &one[stride * e + mat * x];
                double *dst = Pc + stride * e + mat * x;
                for (size_t k = 0; k < mat; ++k) dst[k] = f * src[k];
            }
    }
}

}  // namespace pgm
