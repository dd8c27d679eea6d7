// treelik_rates_test.cpp — tree_likelihood_rates_host and gamma_rates (host/treelik_rates.cpp) on cases read from a file, the results
// printed as hexadecimal floats (%a: every bit) for tests/test_cpu_mlgamma.py to compare with tests/treelik_rates_ref.py.  Host code
// only; built once plainly and once under AddressSanitizer and UBSan.
//
// The file: the number of cases, then per case `dim nleaves nnodes ncols derivs ncat`, the nnodes parents, the nleaves x ncols row
// values, the dim frequencies, the ncat weights and the ncat x (nnodes - 1) x {3 or 1} x dim x dim matrix entries (floats as %a); then
// the number of (alpha, K) pairs and the pairs.  Per case one line each of site_l, site_k, post, d1 and d2 (every output preset: d1 and
// d2 are untouched without derivs, all of them by a rejection), or `rejected <message>`; per pair one line of K rates.
#include "pgm_host.h"

#include <cstdio>
#include <vector>

using namespace pgm;

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: treelik_rates_test <cases>\n"); return 1; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        unsigned dim, nleaves, nnodes, ncols, ncat;
        int derivs;
        if (fscanf(f, "%u %u %u %u %d %u", &dim, &nleaves, &nnodes, &ncols, &derivs, &ncat) != 6) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        std::vector<uint32_t> parent(nnodes);
        for (auto &p : parent) { unsigned v; if (fscanf(f, "%u", &v) != 1) return 1; p = v; }
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        for (auto &r : rows) { int v; if (fscanf(f, "%d", &v) != 1) return 1; r = (int8_t)v; }
        const size_t nedges = nnodes > 0 ? nnodes - 1 : 0, held = ncat <= 64 ? ncat : 0;   // (the file holds nothing for a count this far out)
        std::vector<double> pi(dim), w(held), P(held * nedges * (derivs ? 3 : 1) * dim * dim);
        for (auto &v : pi) if (fscanf(f, "%la", &v) != 1) return 1;
        for (auto &v : w) if (fscanf(f, "%la", &v) != 1) return 1;
        for (auto &v : P) if (fscanf(f, "%la", &v) != 1) return 1;
        std::vector<double> site_l(ncols, -7.5), post(held * ncols, -7.5), d1(nedges, -7.5), d2(d1);
        std::vector<int32_t> site_k(ncols, -7);
        try {
            tree_likelihood_rates_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), derivs, site_l.data(), site_k.data(),
                                       post.data(), d1.data(), d2.data());
        } catch (pgm_exception &e) {
            bool untouched = true;
            for (double v : site_l) untouched = untouched && v == -7.5;
            for (double v : post) untouched = untouched && v == -7.5;
            for (double v : d1) untouched = untouched && v == -7.5;
            for (int32_t v : site_k) untouched = untouched && v == -7;
            printf("rejected%s %s\n", untouched ? "" : " (outputs written)", e.what());
            continue;
        }
        for (double v : site_l) printf("%a ", v);
        printf("\n");
        for (int32_t v : site_k) printf("%d ", v);
        printf("\n");
        for (double v : post) printf("%a ", v);
        printf("\n");
        for (double v : d1) printf("%a ", v);
        printf("\n");
        for (double v : d2) printf("%a ", v);
        printf("\n");
    }
    int npairs = 0;
    if (fscanf(f, "%d", &npairs) != 1) return 1;
    for (int k = 0; k < npairs; ++k) {
        double alpha;
        unsigned K;
        if (fscanf(f, "%la %u", &alpha, &K) != 2) return 1;
        for (double v : gamma_rates(alpha, K)) printf("%a ", v);
        printf("\n");
    }
    fclose(f);
    printf("ok %d cases %d pairs\n", ncases, npairs);
    return 0;
}
