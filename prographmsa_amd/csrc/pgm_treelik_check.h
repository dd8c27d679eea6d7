// pgm_treelik_check.h — what the tree-likelihood entries refuse past their null pointers, once for the C ABI (pgm_treelik_capi.inc,
// which wraps a message in fail(PGM_ERR_INVALID, ...)) and for the host statements (host/treelik*.cpp, which wrap it in error(...)).
// Plain C++: arguments and structure only, no likelihood arithmetic.  Every function returns an empty string or the message.
#ifndef PGM_TREELIK_CHECK_H_
#define PGM_TREELIK_CHECK_H_

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pgm_hip.h"

// ncat and the categories' weights (pgm_tree_likelihood_rates, pgm_tree_ancestral, pgm_tree_nni)
inline std::string pgm_treelik_check_rates(uint32_t ncat, const double *w) {
    if (ncat < 1 || ncat > PGM_TREELIK_MAXCAT) return "tree likelihood: ncat must be 1 .. " + std::to_string(PGM_TREELIK_MAXCAT);
    for (uint32_t c = 0; c < ncat; ++c)
        if (!(w[c] > 0.0 && w[c] < INFINITY)) return "tree likelihood: weight " + std::to_string(c) + " is not finite and above 0";
    return std::string();
}

// The sizes, the tree and the rows (include/pgm_hip.h: pgm_tree_likelihood), and the children of every node in ascending order:
// `tree` gets child_off (nnodes + 1), then child (nnodes - 1).
inline std::string pgm_treelik_check_tree(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                          std::vector<uint32_t> &tree) {
    const std::string w = "tree likelihood: ";
    if (dim < 1 || dim > 64) return w + "dim must be 1 .. 64";
    if (nleaves < 2 || ncols == 0 || nnodes <= nleaves) return w + "nleaves must be at least 2, ncols at least 1 and nnodes above nleaves";
    tree.assign((size_t)nnodes + 1, 0);
    uint32_t roots = 0;
    for (uint32_t v = 0; v < nnodes; ++v) {
        if (parent[v] == UINT32_MAX) { ++roots; continue; }
        if (parent[v] <= v || parent[v] >= nnodes) return w + "the parent of node " + std::to_string(v) + " is not above it";
        if (parent[v] < nleaves) return w + "leaf " + std::to_string(parent[v]) + " is a parent";
        ++tree[parent[v] + 1];
    }
    if (roots != 1) return w + std::to_string(roots) + " roots";
    for (uint32_t v = nleaves; v < nnodes; ++v)
        if (tree[v + 1] < 2) return w + "inner node " + std::to_string(v) + " has fewer than 2 children";
    for (uint32_t v = 0; v < nnodes; ++v) tree[v + 1] += tree[v];
    const uint32_t nedges = nnodes - 1;   // (every node but the root is a child: tree[nnodes] == nedges)
    tree.resize((size_t)nnodes + 1 + nedges);
    {
        std::vector<uint32_t> fill(tree.begin(), tree.begin() + nnodes);
        for (uint32_t v = 0; v < nnodes; ++v)
            if (parent[v] != UINT32_MAX) tree[(size_t)nnodes + 1 + fill[parent[v]]++] = v;
    }
    const size_t nrow = (size_t)nleaves * ncols;
    for (size_t k = 0; k < nrow; ++k)
        if (rows[k] < -2 || rows[k] >= (int)dim) return w + "row value " + std::to_string((int)rows[k]) + " outside -2 .. dim - 1";
    return std::string();
}

// the candidates of pgm_tree_nni on a tree that passed pgm_treelik_check_tree
inline std::string pgm_treelik_check_candidates(uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a,
                                                const uint32_t *cand_c) {
    if (ncand == 0) return "tree nni: no candidate";
    for (uint32_t q = 0; q < ncand; ++q) {
        const uint32_t v = cand_v[q], a = cand_a[q], c = cand_c[q];
        const std::string what = "tree nni: candidate " + std::to_string(q) + ": ";
        if (v >= nnodes || v < nleaves || parent[v] == UINT32_MAX) return what + "v is not an inner node below the root";
        if (a >= nnodes || parent[a] != v) return what + "a is not a child of v";
        if (c >= nnodes || c == v || parent[c] != parent[v]) return what + "c is not another child of the parent of v";
    }
    return std::string();
}

// The candidates of pgm_tree_spr on a tree that passed pgm_treelik_check_tree (child_off: the start of its children lists).  `path`
// gets PGM_TREELIK_SPR_STRIDE values per candidate: J, M, then the J + M + 1 nodes a_0 = p .. a_J = a, c_1 .. c_M = y of the
// interface's path (the rest of the stride is 0).
#define PGM_TREELIK_SPR_STRIDE (PGM_TREE_SPR_MAXPATH + 4)
inline std::string pgm_treelik_check_spr(uint32_t nnodes, const uint32_t *parent, const uint32_t *child_off, uint32_t ncand, const uint32_t *cand_v,
                                         const uint32_t *cand_y, std::vector<uint32_t> &path) {
    if (ncand == 0) return "tree spr: no candidate";
    path.assign((size_t)ncand * PGM_TREELIK_SPR_STRIDE, 0);
    for (uint32_t q = 0; q < ncand; ++q) {
        const uint32_t v = cand_v[q], y = cand_y[q];
        const std::string what = "tree spr: candidate " + std::to_string(q) + ": ";
        if (v >= nnodes || parent[v] == UINT32_MAX) return what + "v is not a node below the root";
        if (y >= nnodes || parent[y] == UINT32_MAX) return what + "y is not a node below the root";
        const uint32_t p = parent[v], arity = child_off[p + 1] - child_off[p];
        if (arity == 2 && parent[p] == UINT32_MAX) return what + "the parent of v is a root of two children";
        if (arity == 2 && (y == p || parent[y] == p)) return what + "y is the parent or the sibling of v: the tree itself";
        // both ends climb to the lowest common ancestor, the lower numbered first (a parent's number is above its children's)
        uint32_t up[PGM_TREE_SPR_MAXPATH + 1], down[PGM_TREE_SPR_MAXPATH + 1], J = 0, M = 0, x = p, z = y;
        while (x != z) {
            if (J + M == PGM_TREE_SPR_MAXPATH) return what + "a path of more than " + std::to_string(PGM_TREE_SPR_MAXPATH) + " edges";
            if (x < z) { up[J++] = x; x = parent[x]; }
            else {
                if (z == v) return what + "y is in the subtree of v";
                down[M++] = z;
                z = parent[z];
            }
        }
        uint32_t *out = &path[(size_t)q * PGM_TREELIK_SPR_STRIDE];
        out[0] = J; out[1] = M;
        for (uint32_t j = 0; j < J; ++j) out[2 + j] = up[j];
        out[2 + J] = x;
        for (uint32_t m = 0; m < M; ++m) out[2 + J + 1 + m] = down[M - 1 - m];
    }
    return std::string();
}

#endif
