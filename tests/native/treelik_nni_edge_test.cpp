// treelik_nni_edge_test.cpp — tree_nni_edge_host and ml_nni_edge_lengths (host/treelik_nni.cpp) on cases read from a file, the results
// printed as hexadecimal floats (%a: every bit) for tests/test_cpu_mlnniopt.py to compare with tests/treelik_nni_edge_ref.py.  Host
// code only; built once plainly and once under AddressSanitizer and UBSan.
//
// The file is binary, in the machine's byte order: an int32 number of cases, then per case eight int32 `dim nleaves nnodes ncols ncat
// ncand rounds null`, the nnodes uint32 parents, the nleaves x ncols int8 row values, as doubles the dim frequencies, the ncat weights
// and the ncat x (nnodes - 1) x dim x dim matrix entries, and the ncand x 3 uint32 candidates (v, a, c).  Then with rounds == 0 the
// ncat x ncand x 3 x dim x dim doubles of Pc, and one line each of site_l, site_k, post, rho, d1, d2 is printed (every output preset;
// null: 1, 2, 3 pass a null Pc, d1, d2); with rounds > 0 the nnodes - 1 lengths and the matrices A and B (ncat x dim x dim each,
// column-major) of the family Z(t) = (A + t B) / (1 + t), whose three matrices per trial length are formed here in + - * / as
// treelik_nni_edge_ref.rational_matrices forms them, and one line each of t_opt, gain_opt and the rho rows is printed.  A refusal prints
// `rejected <message>`.  Further arguments: the bytes of partials and outside vectors tree_nni_edge_host holds at a time (1: a block
// per column chunk; 0: the default), and the bytes of Pc per call of the optimiser (1: one candidate per group).
#include "pgm_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pgm;

template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
static void line(const std::vector<double> &v, size_t n) { for (size_t j = 0; j < n; ++j) printf("%a ", v[j]); printf("\n"); }

int main(int argc, char **argv) {
    if (argc < 2 || argc > 4) { fprintf(stderr, "usage: treelik_nni_edge_test <cases> [block bytes] [pc bytes]\n"); return 1; }
    size_t block_bytes = argc >= 3 ? (size_t)strtoull(argv[2], nullptr, 10) : 0;
    if (block_bytes == 0) block_bytes = kTreelikNniBlockBytes;
    const size_t pc_bytes = argc >= 4 ? (size_t)strtoull(argv[3], nullptr, 10) : kNniEdgeBytes;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        int32_t head[8];
        if (fread(head, 4, 8, f) != 8) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        const uint32_t dim = (uint32_t)head[0], nleaves = (uint32_t)head[1], nnodes = (uint32_t)head[2], ncols = (uint32_t)head[3], ncat = (uint32_t)head[4];
        const uint32_t ncand = (uint32_t)head[5], rounds = (uint32_t)head[6];
        const int null = head[7];
        std::vector<uint32_t> parent(nnodes), cand(3 * (size_t)ncand);
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        const size_t nedges = nnodes > 0 ? nnodes - 1 : 0, held = ncat <= 64 ? ncat : 0, mat = (size_t)dim * dim;
        std::vector<double> pi(dim), w(held), P(held * nedges * mat);
        if (!get(f, parent) || !get(f, rows) || !get(f, pi) || !get(f, w) || !get(f, P) || !get(f, cand)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
        std::vector<double> Pc(rounds ? 0 : held * ncand * 3 * mat + 1), lengths(rounds ? nedges : 0), A(rounds ? held * mat : 0), B(A.size());
        if (!rounds) { Pc.pop_back(); if (!get(f, Pc)) return 1; Pc.push_back(0.0); }   // (one entry more, so it is never null by itself)
        else if (!get(f, lengths) || !get(f, A) || !get(f, B)) return 1;
        std::vector<uint32_t> cv(ncand + 1), ca(ncand + 1), cc(ncand + 1);
        for (uint32_t q = 0; q < ncand; ++q) { cv[q] = cand[3 * q]; ca[q] = cand[3 * q + 1]; cc[q] = cand[3 * q + 2]; }
        std::vector<double> site_l(ncols, -7.5), post(held * ncols, -7.5), rho((size_t)ncand * ncols + 1, -7.5), d1(ncand + 1, -7.5), d2(ncand + 1, -7.5);
        std::vector<int32_t> site_k(ncols, -7);
        try {
            if (rounds) {
                const MlNniEdgeMatrices family = [&](const std::vector<double> &t, std::vector<double> &out) {
                    out.resize(held * t.size() * 3 * mat);
                    for (size_t c = 0; c < held; ++c)
                        for (size_t q = 0; q < t.size(); ++q) {
                            const double one = 1.0 + t[q], sq = one * one;
                            double *Z = &out[(c * t.size() + q) * 3 * mat];
                            for (size_t e = 0; e < mat; ++e) {
                                const double a = A[c * mat + e], b = B[c * mat + e];
                                Z[e] = (a + t[q] * b) / one;
                                Z[mat + e] = (b - a) / sq;
                                Z[2 * mat + e] = (-2.0 * (b - a)) / (sq * one);
                            }
                        }
                };
                const MlNniEdgeResult r = ml_nni_edge_lengths(family, dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), lengths, ncand,
                                                              cv.data(), ca.data(), cc.data(), rounds, nullptr, pc_bytes);
                line(r.t_opt, r.t_opt.size());
                line(r.gain_opt, r.gain_opt.size());
                line(r.rho, r.rho.size());
                continue;
            }
            tree_nni_edge_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), ncand, cv.data(), ca.data(), cc.data(),
                               null == 1 ? nullptr : Pc.data(), site_l.data(), site_k.data(), post.data(), rho.data(), null == 2 ? nullptr : d1.data(),
                               null == 3 ? nullptr : d2.data(), block_bytes);
        } catch (pgm_exception &e) {
            bool untouched = true;
            for (double v : site_l) untouched = untouched && v == -7.5;
            for (double v : post) untouched = untouched && v == -7.5;
            for (double v : rho) untouched = untouched && v == -7.5;
            for (double v : d1) untouched = untouched && v == -7.5;
            for (double v : d2) untouched = untouched && v == -7.5;
            for (int32_t v : site_k) untouched = untouched && v == -7;
            printf("rejected%s %s\n", untouched ? "" : " (outputs written)", e.what());
            continue;
        }
        line(site_l, site_l.size());
        for (int32_t v : site_k) printf("%d ", v);
        printf("\n");
        line(post, post.size());
        line(rho, rho.size() - 1);
        line(d1, ncand);
        line(d2, ncand);
    }
    fclose(f);
    printf("ok %d cases\n", ncases);
    return 0;
}
