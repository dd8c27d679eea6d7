// treelik_nni_test.cpp — tree_nni_host and treelik_nni_gain (host/treelik_nni.cpp) on cases read from a file, the results printed as
// hexadecimal floats (%a: every bit) for tests/test_cpu_mlsearch.py to compare with tests/treelik_nni_ref.py.  Host code only; built
// once plainly and once under AddressSanitizer and UBSan.
//
// The file is binary, in the machine's byte order: an int32 number of cases, then per case six int32 `dim nleaves nnodes ncols ncat
// ncand`, the nnodes uint32 parents, the nleaves x ncols int8 row values, as doubles the dim frequencies, the ncat weights and the
// ncat x (nnodes - 1) x dim x dim matrix entries, and the ncand x 3 uint32 candidates (v, a, c).  Per case one line each of site_l,
// site_k, post, rho and the gains (every output preset), or `rejected <message>`.  A second argument is the bytes of partials and
// outside vectors tree_nni_host holds at a time (1: a block per column chunk).
#include "pgm_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pgm;

template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 2 && argc != 3) { fprintf(stderr, "usage: treelik_nni_test <cases> [block bytes]\n"); return 1; }
    const size_t block_bytes = argc == 3 ? (size_t)strtoull(argv[2], nullptr, 10) : kTreelikNniBlockBytes;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        int32_t head[6];
        if (fread(head, 4, 6, f) != 6) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        const uint32_t dim = (uint32_t)head[0], nleaves = (uint32_t)head[1], nnodes = (uint32_t)head[2], ncols = (uint32_t)head[3], ncat = (uint32_t)head[4];
        const uint32_t ncand = (uint32_t)head[5];
        std::vector<uint32_t> parent(nnodes), cand(3 * (size_t)ncand);
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        const size_t nedges = nnodes > 0 ? nnodes - 1 : 0, held = ncat <= 64 ? ncat : 0;   // (the file holds nothing for a count this far out)
        std::vector<double> pi(dim), w(held), P(held * nedges * dim * dim);
        if (!get(f, parent) || !get(f, rows) || !get(f, pi) || !get(f, w) || !get(f, P) || !get(f, cand)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
        std::vector<uint32_t> cv(ncand + 1), ca(ncand + 1), cc(ncand + 1);   // (never null: ncand == 0 is refused for what it is)
        for (uint32_t q = 0; q < ncand; ++q) { cv[q] = cand[3 * q]; ca[q] = cand[3 * q + 1]; cc[q] = cand[3 * q + 2]; }
        std::vector<double> site_l(ncols, -7.5), post(held * ncols, -7.5), rho((size_t)ncand * ncols + 1, -7.5), gain(ncand, -7.5);   // (rho: one entry more, so it is never null)
        std::vector<int32_t> site_k(ncols, -7);
        try {
            tree_nni_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), ncand, cv.data(), ca.data(), cc.data(), site_l.data(),
                          site_k.data(), post.data(), rho.data(), block_bytes);
            treelik_nni_gain(ncand, ncols, rho.data(), gain.data());
        } catch (pgm_exception &e) {
            bool untouched = true;
            for (double v : site_l) untouched = untouched && v == -7.5;
            for (double v : post) untouched = untouched && v == -7.5;
            for (double v : rho) untouched = untouched && v == -7.5;
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
        for (size_t j = 0; j + 1 < rho.size(); ++j) printf("%a ", rho[j]);
        printf("\n");
        for (double v : gain) printf("%a ", v);
        printf("\n");
    }
    fclose(f);
    printf("ok %d cases\n", ncases);
    return 0;
}
