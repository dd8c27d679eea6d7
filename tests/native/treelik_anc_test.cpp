// treelik_anc_test.cpp — tree_ancestral_host and tree_ancestral_presence (host/treelik_anc.cpp) on cases read from a file, the results
// printed as hexadecimal floats (%a: every bit) for tests/test_cpu_mlancestral.py to compare with tests/treelik_anc_ref.py.  Host code
// only; built once plainly and once under AddressSanitizer and UBSan.
//
// The file is binary, in the machine's byte order (the cases of 61 and 64 states with 16 categories hold 0.9 million matrix entries
// each: as text the file would be some 200 MB): an int32 number of cases, then per case six int32 `dim nleaves nnodes ncols ncat
// full`, the nnodes uint32 parents, the nleaves x ncols int8 row values, and as doubles the dim frequencies, the ncat weights and the
// ncat x (nnodes - 1) x dim x dim matrix entries.  Per case one line each of site_l, site_k, post, anc_state, anc_prob, anc_post
// (every output preset; without `full` the entry gets no anc_post and the line shows the preset values) and the presence of every
// inner node at every column, or `rejected <message>`.
#include "pgm_host.h"

#include <cstdio>
#include <vector>

using namespace pgm;

template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: treelik_anc_test <cases>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        int32_t head[6];
        if (fread(head, 4, 6, f) != 6) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        const uint32_t dim = (uint32_t)head[0], nleaves = (uint32_t)head[1], nnodes = (uint32_t)head[2], ncols = (uint32_t)head[3], ncat = (uint32_t)head[4];
        const int full = head[5];
        std::vector<uint32_t> parent(nnodes);
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        const size_t nedges = nnodes > 0 ? nnodes - 1 : 0, held = ncat <= 64 ? ncat : 0;   // (the file holds nothing for a count this far out)
        const size_t ninner = nnodes > nleaves ? nnodes - nleaves : 0;
        std::vector<double> pi(dim), w(held), P(held * nedges * dim * dim);
        if (!get(f, parent) || !get(f, rows) || !get(f, pi) || !get(f, w) || !get(f, P)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
        std::vector<double> site_l(ncols, -7.5), post(held * ncols, -7.5), prob(ninner * ncols, -7.5), anc(ninner * ncols * dim, -7.5);
        std::vector<int32_t> site_k(ncols, -7);
        std::vector<int8_t> state(ninner * ncols, -7);
        std::vector<uint8_t> present(ninner * ncols, 7);
        try {
            tree_ancestral_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), site_l.data(), site_k.data(), post.data(),
                                state.data(), prob.data(), full ? anc.data() : nullptr);
            tree_ancestral_presence(nleaves, nnodes, parent.data(), ncols, rows.data(), present.data());
        } catch (pgm_exception &e) {
            bool untouched = true;
            for (double v : site_l) untouched = untouched && v == -7.5;
            for (double v : post) untouched = untouched && v == -7.5;
            for (double v : prob) untouched = untouched && v == -7.5;
            for (double v : anc) untouched = untouched && v == -7.5;
            for (int32_t v : site_k) untouched = untouched && v == -7;
            for (int8_t v : state) untouched = untouched && v == -7;
            printf("rejected%s %s\n", untouched ? "" : " (outputs written)", e.what());
            continue;
        }
        for (double v : site_l) printf("%a ", v);
        printf("\n");
        for (int32_t v : site_k) printf("%d ", v);
        printf("\n");
        for (double v : post) printf("%a ", v);
        printf("\n");
        for (int8_t v : state) printf("%d ", (int)v);
        printf("\n");
        for (double v : prob) printf("%a ", v);
        printf("\n");
        for (double v : anc) printf("%a ", v);
        printf("\n");
        for (uint8_t v : present) printf("%d", (int)v);
        printf("\n");
    }
    fclose(f);
    printf("ok %d cases\n", ncases);
    return 0;
}
