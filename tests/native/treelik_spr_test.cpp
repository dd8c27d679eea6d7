// treelik_spr_test.cpp — tree_spr_host and the moves of the SPR scan (host/treelik_spr.cpp) on cases read from a file, the results
// printed as hexadecimal floats (%a: every bit) for tests/test_cpu_mlspr.py to compare with tests/treelik_spr_ref.py.  Host code only;
// built once plainly and once under AddressSanitizer and UBSan.
//
// The file is binary, in the machine's byte order: an int32 number of cases, then per case six int32 `dim nleaves nnodes ncols ncat
// ncand`, the nnodes uint32 parents, the nleaves x ncols int8 row values, as doubles the dim frequencies, the ncat weights, the
// ncat x (nnodes - 1) x dim x dim entries of P and as many of Ph, and the ncand x 2 uint32 candidates (v, y).  Per case one line each
// of site_l, site_k, post, rho and the gains (every output preset), or `rejected <message>`.  A second argument is the bytes of
// partials and outside vectors tree_spr_host holds at a time (1: a block per column chunk).
//
// `treelik_spr_test moves <radius> <newick>`: the candidates of the tree within the radius (ml_spr_candidates), then for a number of
// seeded gain orders the greedy pick by disjoint touched sets (ml_spr_touched) applied at once (ml_spr_apply): the new tree must pass
// ml_tree_topology with the same leaves and one node more or as many.  Prints `moves ok <candidates> <sets> <moves applied>`.
#include "pgm_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <sstream>
#include <vector>

using namespace pgm;

template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int moves(uint32_t radius, const char *text) {
    std::istringstream in(text);
    std::unique_ptr<PhyTree> tree(parse_newick(in));
    const MlTreeTopology topo = ml_tree_topology(*tree);
    std::vector<double> lengths(topo.nnodes - 1);
    for (uint32_t e = 0; e + 1 < topo.nnodes; ++e) lengths[e] = topo.node[e]->getBranchLength();
    std::vector<uint32_t> cv, cy;
    ml_spr_candidates(topo.nnodes, topo.parent.data(), radius, cv, cy);
    if (cv.empty()) { printf("no candidate\n"); return 1; }
    std::mt19937 rng(7);
    size_t sets = 0, applied = 0;
    for (int round = 0; round < 40; ++round) {
        std::vector<uint32_t> order(cv.size());
        std::iota(order.begin(), order.end(), 0u);
        std::shuffle(order.begin(), order.end(), rng);
        std::vector<char> used(topo.nnodes, 0);
        std::vector<uint32_t> pv, py;
        for (uint32_t q : order) {
            const std::vector<uint32_t> touched = ml_spr_touched(topo.nnodes, topo.parent.data(), cv[q], cy[q]);
            if (std::any_of(touched.begin(), touched.end(), [&](uint32_t x) { return used[x] != 0; })) continue;
            for (uint32_t x : touched) used[x] = 1;
            pv.push_back(cv[q]); py.push_back(cy[q]);
        }
        for (size_t m = pv.size(); m >= 1; m = m / 2) {
            std::unique_ptr<PhyTree> next(ml_spr_apply(topo, lengths, (uint32_t)m, pv.data(), py.data()));
            const MlTreeTopology nt = ml_tree_topology(*next);
            if (nt.names != topo.names || nt.nleaves != topo.nleaves) { printf("round %d: the leaves changed\n", round); return 1; }
            if (nt.nnodes < topo.nnodes || nt.nnodes > topo.nnodes + m) { printf("round %d: %u nodes from %u\n", round, nt.nnodes, topo.nnodes); return 1; }
            for (uint32_t e = 0; e + 1 < nt.nnodes; ++e) {
                const double t = nt.node[e]->getBranchLength();
                if (!(t >= kMlMinLength / 2 && t <= kMlMaxLength)) { printf("round %d: length %g\n", round, t); return 1; }
            }
            ++sets;
            applied += m;
        }
    }
    printf("moves ok %zu %zu %zu\n", cv.size(), sets, applied);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "moves") == 0) {
        try { return moves((uint32_t)atoi(argv[2]), argv[3]); }
        catch (pgm_exception &e) { printf("error %s\n", e.what()); return 1; }
    }
    if (argc != 2 && argc != 3) { fprintf(stderr, "usage: treelik_spr_test <cases> [block bytes] | moves <radius> <newick>\n"); return 1; }
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
        std::vector<uint32_t> parent(nnodes), cand(2 * (size_t)ncand);
        std::vector<int8_t> rows((size_t)nleaves * ncols);
        const size_t nedges = nnodes > 0 ? nnodes - 1 : 0, held = ncat <= 64 ? ncat : 0;   // (the file holds nothing for a count this far out)
        std::vector<double> pi(dim), w(held), P(held * nedges * dim * dim), Ph(P.size());
        if (!get(f, parent) || !get(f, rows) || !get(f, pi) || !get(f, w) || !get(f, P) || !get(f, Ph) || !get(f, cand)) { fprintf(stderr, "case %d: truncated\n", k); return 1; }
        std::vector<uint32_t> cv(ncand + 1), cy(ncand + 1);   // (never null: ncand == 0 is refused for what it is)
        for (uint32_t q = 0; q < ncand; ++q) { cv[q] = cand[2 * q]; cy[q] = cand[2 * q + 1]; }
        std::vector<double> site_l(ncols, -7.5), post(held * ncols, -7.5), rho((size_t)ncand * ncols + 1, -7.5), gain(ncand, -7.5);   // (rho: one entry more, so it is never null)
        std::vector<int32_t> site_k(ncols, -7);
        try {
            tree_spr_host(dim, nleaves, nnodes, parent.data(), ncols, rows.data(), pi.data(), ncat, w.data(), P.data(), Ph.data(), ncand, cv.data(), cy.data(), site_l.data(),
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
