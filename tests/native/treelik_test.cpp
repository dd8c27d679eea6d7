// treelik_test.cpp — tree_likelihood_host (host/treelik.cpp) on cases read from a file, the results printed as hexadecimal floats
// (%a: every bit) for tests/test_cpu_mltree.py to compare with tests/treelik_ref.py.  Host code only; built once plainly and once
// under AddressSanitizer and UBSan.
//
// The file: the number of cases, then per case `dim nleaves nnodes ncols derivs`, the nnodes parents, the nleaves x ncols row
// values, the dim frequencies and the (nnodes - 1) x {3 or 1} x dim x dim matrix entries (floats as %a).  Per case one line each of
// site_l, site_k, d1 and d2 (the latter two preset to -7.5: untouched without derivs), or `rejected <message>`.
#include "pgm_host.h"

#include <cstdio>
#include <vector>

using namespace pgm;

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: treelik_test <cases>\n"); return 1; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        unsigned dim, nleaves, nnodes, ncols;
        int derivs;
        if (fscanf(f, "%u %u %u %u %d", &dim, &nleaves, &nnodes, &ncols, &derivs) != 5) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        std::vector<uint32_t> parent(nnodes);
        for (auto &p : parent) { unsigned v; if (fscanf(f, "%u", &v) != 1) return 1; p = v; }
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        for (auto &r : rows) { int v; if (fscanf(f, "%d", &v) != 1) return 1; r = (int8_t)v; }
        std::vector<double> pi(dim), P((size_t)(nnodes > 0 ? nnodes - 1 : 0) * (derivs ? 3 : 1) * dim * dim);
        for (auto &v : pi) if (fscanf(f, "%la", &v) != 1) return 1;
        for (auto &v : P) if (fscanf(f, "%la", &v) != 1) return 1;
        std::vector<double> site_l(ncols, -7.5), d1(nnodes > 0 ? nnodes - 1 : 0, -7.5), d2(d1);
        std::vector<int32_t> site_k(ncols, -7);
        try {
            tree_likelihood_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), P.data(), derivs, site_l.data(), site_k.data(), d1.data(), d2.data());
        } catch (pgm_exception &e) {
            printf("rejected %s\n", e.what());
            continue;
        }
        for (double v : site_l) printf("%a ", v);
        printf("\n");
        for (int32_t v : site_k) printf("%d ", v);
        printf("\n");
        for (double v : d1) printf("%a ", v);
        printf("\n");
        for (double v : d2) printf("%a ", v);
        printf("\n");
    }
    fclose(f);
    printf("ok %d cases\n", ncases);
    return 0;
}
