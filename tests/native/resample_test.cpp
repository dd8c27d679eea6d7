// resample_test.cpp — resampled_sums_host, bootstrap_columns and ml_branch_support (host/treelik_support.cpp, pgm_host.h) on cases read
// from a file, the results printed as hexadecimal floats (%a: every bit) for tests/test_cpu_mlsupport.py to compare with
// tests/resample_ref.py.  Host code only; built once plainly and once under AddressSanitizer and UBSan.
//
// The file is binary, in the machine's byte order: an int32 number of cases, then per case an int32 kind and
//   kind 0, the sums: six int32 `nrow ncols nrep nx ncolumns nulls`, nx doubles of x and ncolumns uint32 of cols (what the file holds of
//     them: a call that is refused for its sizes reads neither), nulls a mask of the pointers passed as null (1 x, 2 cols, 4 out).
//     One line of out (preset), or `rejected <message>`.
//   kind 1, the columns: three int32 `nrep ncols seed`.  One line of the nrep x ncols columns.
//   kind 2, the support: seven int32 `dim nleaves nnodes ncols ncat nrep xbytes`, the nnodes uint32 parents, the nleaves x ncols int8 row
//     values, as doubles the dim frequencies, the ncat weights and the ncat x (nnodes - 1) x dim x dim matrix entries, and the nrep x
//     ncols uint32 columns.  A line `node candidates alrt sh_hits rell_hits` per supported node, then `end <nodes>`.
#include "pgm_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pgm;

template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: resample_test <cases>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        int32_t kind = -1;
        if (fread(&kind, 4, 1, f) != 1) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        if (kind == 0) {
            int32_t head[6];
            if (fread(head, 4, 6, f) != 6) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
            const uint32_t nrow = (uint32_t)head[0], ncols = (uint32_t)head[1], nrep = (uint32_t)head[2], nulls = (uint32_t)head[5];
            std::vector<double> x((size_t)head[3] + 1);   // (one entry more: never null for being empty)
            std::vector<uint32_t> cols((size_t)head[4] + 1);
            x.pop_back(); cols.pop_back();
            if (!get(f, x) || !get(f, cols)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
            x.push_back(0.0); cols.push_back(0);
            const size_t nout = (size_t)head[3] == (size_t)nrow * ncols && (size_t)head[4] == (size_t)nrep * ncols ? (size_t)nrow * nrep : 16;
            std::vector<double> out(nout + 1, -7.5);
            try {
                resampled_sums_host(nrow, ncols, nulls & 1 ? nullptr : x.data(), nrep, nulls & 2 ? nullptr : cols.data(), nulls & 4 ? nullptr : out.data());
            } catch (pgm_exception &e) {
                bool untouched = true;
                for (double v : out) untouched = untouched && v == -7.5;
                printf("rejected%s %s\n", untouched ? "" : " (out written)", e.what());
                continue;
            }
            for (size_t j = 0; j < nout; ++j) printf("%a ", out[j]);
            printf("\n");
        } else if (kind == 1) {
            int32_t head[3];
            if (fread(head, 4, 3, f) != 3) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
            for (uint32_t c : bootstrap_columns((uint32_t)head[0], (uint32_t)head[1], (uint64_t)head[2])) printf("%u ", c);
            printf("\n");
        } else if (kind == 2) {
            int32_t head[7];
            if (fread(head, 4, 7, f) != 7) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
            const uint32_t dim = (uint32_t)head[0], nleaves = (uint32_t)head[1], nnodes = (uint32_t)head[2], ncols = (uint32_t)head[3], ncat = (uint32_t)head[4];
            const uint32_t nrep = (uint32_t)head[5];
            std::vector<uint32_t> parent(nnodes), cols((size_t)nrep * ncols);
            std::vector<int8_t> rows((size_t)nleaves * ncols);
            std::vector<double> pi(dim), w(ncat), P((size_t)ncat * (nnodes - 1) * dim * dim);
            if (!get(f, parent) || !get(f, rows) || !get(f, pi) || !get(f, w) || !get(f, P) || !get(f, cols)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
            const std::vector<MlSupportNode> nodes = ml_branch_support(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), nrep,
                                                                       cols.data(), nullptr, (size_t)head[6]);
            for (const MlSupportNode &s : nodes) printf("%u %u %a %u %u\n", s.node, s.candidates, s.alrt, s.sh_hits, s.rell_hits);
            printf("end %zu\n", nodes.size());
        } else { fprintf(stderr, "case %d: unknown kind %d\n", k, kind); return 1; }
    }
    fclose(f);
    printf("ok %d cases\n", ncases);
    return 0;
}
