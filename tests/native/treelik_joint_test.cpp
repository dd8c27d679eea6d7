// treelik_joint_test.cpp — tree_ancestral_joint_host and tree_ancestral_sample_host (host/treelik_joint.cpp) on cases read from a file,
// the results printed with hexadecimal floats (%a: every bit) for tests/test_cpu_mljoint.py to compare with tests/treelik_joint_ref.py.
// Host code only; built once plainly and once under AddressSanitizer and UBSan.
//
// The file is binary, in the machine's byte order: an int32 number of cases, then per case seven int32 `dim nleaves nnodes ncols ncat
// nsamp which` (which: 1 the joint entry, 2 the sampler, 3 both), two uint64 `first_sample seed`, the nnodes uint32 parents, the
// nleaves x ncols int8 row values, and as doubles the dim frequencies, the ncat weights and the ncat x (nnodes - 1) x dim x dim matrix
// entries.  Per case and entry one line each of site_l, site_k, post and then cat, joint_state, joint_l, joint_k or samp_cat, samp_state
// (every output preset), or `rejected <message>`.
#include "pgm_host.h"

#include <cstdio>
#include <vector>

using namespace pgm;

template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T> static void ints(const std::vector<T> &v, size_t n) { for (size_t k = 0; k < n; ++k) printf("%d ", (int)v[k]); printf("\n"); }
template <class T> static void ints(const std::vector<T> &v) { ints(v, v.size()); }
static void floats(const std::vector<double> &v) { for (double x : v) printf("%a ", x); printf("\n"); }
template <class T> static bool all_are(const std::vector<T> &v, T x) { for (T y : v) if (!(y == x)) return false; return true; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: treelik_joint_test <cases>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < ncases; ++k) {
        int32_t head[7];
        uint64_t draw[2];
        if (fread(head, 4, 7, f) != 7 || fread(draw, 8, 2, f) != 2) { fprintf(stderr, "case %d: bad header\n", k); return 1; }
        const uint32_t dim = (uint32_t)head[0], nleaves = (uint32_t)head[1], nnodes = (uint32_t)head[2], ncols = (uint32_t)head[3], ncat = (uint32_t)head[4];
        const uint32_t nsamp = (uint32_t)head[5];
        const int which = head[6];
        std::vector<uint32_t> parent(nnodes);
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        const size_t nedges = nnodes > 0 ? nnodes - 1 : 0, held = ncat <= 64 ? ncat : 0;   // (the file holds nothing for a count this far out)
        const size_t ninner = nnodes > nleaves ? nnodes - nleaves : 0;
        std::vector<double> pi(dim), w(held), P(held * nedges * dim * dim);
        if (!get(f, parent) || !get(f, rows) || !get(f, pi) || !get(f, w) || !get(f, P)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
        for (int entry = 1; entry <= 2; ++entry) {
            if (!(which & entry)) continue;
            std::vector<double> site_l(ncols, -7.5), post(held * ncols, -7.5), joint_l(ncols, -7.5);
            std::vector<int32_t> site_k(ncols, -7), joint_k(ncols, -7);
            // (one entry more than the entry writes: no sample at all still has a buffer to refuse, and the entry stays within its own)
            const size_t ncat_samp = (size_t)ncols * nsamp, nstate_samp = ninner * ncols * nsamp;
            std::vector<uint8_t> cat(ncols, 77), samp_cat(ncat_samp + 1, 77);
            std::vector<int8_t> state(ninner * ncols, -7), samp_state(nstate_samp + 1, -7);
            try {
                if (entry == 1)
                    tree_ancestral_joint_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), site_l.data(), site_k.data(),
                                              post.data(), cat.data(), state.data(), joint_l.data(), joint_k.data());
                else
                    tree_ancestral_sample_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), nsamp, draw[0], draw[1],
                                               site_l.data(), site_k.data(), post.data(), samp_cat.data(), samp_state.data());
            } catch (pgm_exception &e) {
                const bool untouched = all_are(site_l, -7.5) && all_are(post, -7.5) && all_are(joint_l, -7.5) && all_are(site_k, (int32_t)-7) && all_are(joint_k, (int32_t)-7) &&
                                       all_are(cat, (uint8_t)77) && all_are(samp_cat, (uint8_t)77) && all_are(state, (int8_t)-7) && all_are(samp_state, (int8_t)-7);
                printf("rejected%s %s\n", untouched ? "" : " (outputs written)", e.what());
                continue;
            }
            floats(site_l);
            ints(site_k);
            floats(post);
            if (entry == 1) { ints(cat); ints(state); floats(joint_l); ints(joint_k); }
            else {
                if (samp_cat[ncat_samp] != 77 || samp_state[nstate_samp] != -7) { fprintf(stderr, "case %d: a write past the samples\n", k); return 1; }
                ints(samp_cat, ncat_samp);
                ints(samp_state, nstate_samp);
            }
        }
    }
    fclose(f);
    printf("ok %d cases\n", ncases);
    return 0;
}
