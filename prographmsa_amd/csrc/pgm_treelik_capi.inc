// pgm_treelik_capi.inc — C ABI of the tree likelihood of pgmsa --ml_tree (included by pgm_capi.hip).
// The arguments are checked on the host and the children lists are built there, then: one upload of the tree, the rows, pi and the
// matrices, one launch of pgm_treelik_kernel (a workgroup per block of sites walks the whole tree), with derivs one launch of
// pgm_treelik_sums_kernel, one copy back.  Stateless: nothing of a call is read by the next.
extern "C" float pgm_treelik_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->treelik_ms : 0.0f; }

// The checks both entries share past their pointers, and the children of every node in ascending order: `tree` gets child_off
// (nnodes + 1), then child (nnodes - 1).
static int treelik_tree(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, std::vector<uint32_t> &tree) {
    const std::string w = "tree likelihood: ";
    if (dim < 1 || dim > 64) return fail(PGM_ERR_INVALID, w + "dim must be 1 .. 64");
    if (nleaves < 2 || ncols == 0 || nnodes <= nleaves) return fail(PGM_ERR_INVALID, w + "nleaves must be at least 2, ncols at least 1 and nnodes above nleaves");
    tree.assign((size_t)nnodes + 1, 0);
    uint32_t roots = 0;
    for (uint32_t v = 0; v < nnodes; ++v) {
        if (parent[v] == UINT32_MAX) { ++roots; continue; }
        if (parent[v] <= v || parent[v] >= nnodes) return fail(PGM_ERR_INVALID, w + "the parent of node " + std::to_string(v) + " is not above it");
        if (parent[v] < nleaves) return fail(PGM_ERR_INVALID, w + "leaf " + std::to_string(parent[v]) + " is a parent");
        ++tree[parent[v] + 1];
    }
    if (roots != 1) return fail(PGM_ERR_INVALID, w + std::to_string(roots) + " roots");
    for (uint32_t v = nleaves; v < nnodes; ++v)
        if (tree[v + 1] < 2) return fail(PGM_ERR_INVALID, w + "inner node " + std::to_string(v) + " has fewer than 2 children");
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
        if (rows[k] < -2 || rows[k] >= (int)dim) return fail(PGM_ERR_INVALID, w + "row value " + std::to_string((int)rows[k]) + " outside -2 .. dim - 1");
    return PGM_OK;
}

extern "C" int pgm_tree_likelihood(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                   const double *pi, const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !P || !site_l || !site_k || (derivs && (!d1 || !d2))) return fail(PGM_ERR_INVALID, "null argument");
    std::vector<uint32_t> tree;   // child_off, then child
    if (const int rc = treelik_tree(dim, nleaves, nnodes, parent, ncols, rows, tree)) return rc;
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves;
    const size_t nrow = (size_t)nleaves * ncols;

    const size_t mat = (size_t)dim * dim, p_bytes = 8 * mat * (derivs ? 3 : 1) * nedges;
    const size_t tree_bytes = 4 * tree.size(), pi_off = (tree_bytes + 7) / 8 * 8, rows_off = pi_off + 8 * (size_t)dim;
    const size_t u_count = (size_t)ninner * ncols * dim, nchunks = ((size_t)ncols + PGM_TREELIK_CHUNK - 1) / PGM_TREELIK_CHUNK;
    const size_t g_count = (size_t)nedges * ncols, part_count = 2 * (size_t)nedges * nchunks;
    const size_t l_bytes = 8 * (size_t)ncols, k_bytes = (4 * (size_t)ncols + 7) / 8 * 8, d_bytes = 8 * (size_t)nedges;
    StageCall c(ctx, "tree likelihood", &ctx->treelik_ms);
    uint8_t *d_tree = nullptr, *d_out = nullptr; double *d_P = nullptr, *d_U = nullptr, *d_g = nullptr;
    c.buf(pgm_ctx::SC_TREELIK_TREE, rows_off + nrow, &d_tree);
    c.buf(pgm_ctx::SC_TREELIK_P, p_bytes, &d_P);
    c.buf(pgm_ctx::SC_TREELIK_U, 8 * u_count * (derivs ? 2 : 1), &d_U);
    if (derivs) c.buf(pgm_ctx::SC_TREELIK_G, 8 * (2 * g_count + part_count), &d_g);
    c.buf(pgm_ctx::SC_TREELIK_OUT, l_bytes + k_bytes + 2 * d_bytes, &d_out);
    c.up(d_tree, tree.data(), tree_bytes);
    c.up(d_tree + pi_off, pi, 8 * (size_t)dim);
    c.up(d_tree + rows_off, rows, nrow);
    c.up(d_P, P, p_bytes);

    PgmTreelikArgs a;
    a.dim = dim; a.nleaves = nleaves; a.nnodes = nnodes; a.ncols = ncols; a.spb = PGM_TREELIK_THREADS / dim; a.derivs = derivs ? 1 : 0;
    a.child_off = (const uint32_t *)d_tree; a.child = a.child_off + nnodes + 1;
    a.pi = (const double *)(d_tree + pi_off); a.rows = (const int8_t *)(d_tree + rows_off); a.P = d_P;
    a.U = d_U; a.O = derivs ? d_U + u_count : nullptr;
    a.g = derivs ? d_g : nullptr; a.h = derivs ? d_g + g_count : nullptr;
    a.site_l = (double *)d_out; a.site_k = (int32_t *)(d_out + l_bytes);
    double *d_d1 = (double *)(d_out + l_bytes + k_bytes), *d_d2 = d_d1 + nedges;
    const uint32_t blocks = (uint32_t)(((uint64_t)ncols + a.spb - 1) / a.spb);
    if (c.begin()) {
        hipLaunchKernelGGL(pgm_treelik_kernel, dim3(blocks), dim3(PGM_TREELIK_THREADS), 0, c.s, a);
        if (derivs)
            hipLaunchKernelGGL(pgm_treelik_sums_kernel, dim3(nedges), dim3(PGM_TREELIK_THREADS), 0, c.s, (const double *)a.g, (const double *)a.h, ncols, (uint32_t)nchunks,
                               d_g + 2 * g_count, d_d1, d_d2);
    }
    c.end();
    c.down(site_l, a.site_l, l_bytes);
    c.down(site_k, a.site_k, 4 * (size_t)ncols);
    if (derivs) {
        c.down(d1, d_d1, d_bytes);
        c.down(d2, d_d2, d_bytes);
    }
    return c.finish();
}
