// Harness of tests/test_cpu_wls.py: reads problems "rows cols Z(row-major) x" from stdin until EOF and prints, per problem,
// the active-set iterations and d of pgm::nnls::solve (prographmsa_amd/host/nnls.h), one line, %.17g.
#include <cstdio>
#include <vector>

#include "nnls.h"

int main() {
    int rows, cols;
    while (scanf("%d %d", &rows, &cols) == 2) {
        std::vector<double> Z((size_t)rows * cols), x(rows), d(cols);
        for (double &v : Z) if (scanf("%lf", &v) != 1) return 1;
        for (double &v : x) if (scanf("%lf", &v) != 1) return 1;
        const int iters = pgm::nnls::solve(rows, cols, Z.data(), x.data(), d.data());
        printf("%d", iters);
        for (double v : d) printf(" %.17g", v);
        printf("\n");
    }
    return 0;
}
