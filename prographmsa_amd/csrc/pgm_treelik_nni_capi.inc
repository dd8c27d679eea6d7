// pgm_treelik_nni_capi.inc — C ABI of the nearest-neighbour interchange scores on the ML tree, pgmsa --ml_tree --ml_search (included by
// pgm_capi.hip behind pgm_treelik_anc_capi.inc, whose checks and scratch slots it shares; DESIGN.md 3.20).
// One upload of the tree, the rows, pi, the weights, the parents, the candidates and the matrices of every category; one launch of
// pgm_treelik_nni_walk_kernel over (site block x category), which leaves the partials and the outside vectors in device memory, one
// of pgm_treelik_combine_kernel for site_l, site_k and post, one of pgm_treelik_nni_kernel over (site block x candidate); one copy back.
extern "C" int pgm_tree_nni(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                            const double *pi, uint32_t ncat, const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a,
                            const uint32_t *cand_c, double *site_l, int32_t *site_k, double *post, double *rho) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || !cand_v || !cand_a || !cand_c || !rho) return fail(PGM_ERR_INVALID, "null argument");
    if (ncat < 1 || ncat > PGM_TREELIK_MAXCAT) return fail(PGM_ERR_INVALID, "tree likelihood: ncat must be 1 .. " + std::to_string(PGM_TREELIK_MAXCAT));
    for (uint32_t c = 0; c < ncat; ++c)
        if (!(w[c] > 0.0 && w[c] < INFINITY)) return fail(PGM_ERR_INVALID, "tree likelihood: weight " + std::to_string(c) + " is not finite and above 0");
    std::vector<uint32_t> tree;   // child_off, then child
    if (const int rc = treelik_tree(dim, nleaves, nnodes, parent, ncols, rows, tree)) return rc;
    if (ncand == 0) return fail(PGM_ERR_INVALID, "tree nni: no candidate");
    for (uint32_t q = 0; q < ncand; ++q) {
        const uint32_t v = cand_v[q], a = cand_a[q], c = cand_c[q];
        const std::string what = "tree nni: candidate " + std::to_string(q) + ": ";
        if (v >= nnodes || v < nleaves || parent[v] == UINT32_MAX) return fail(PGM_ERR_INVALID, what + "v is not an inner node below the root");
        if (a >= nnodes || parent[a] != v) return fail(PGM_ERR_INVALID, what + "a is not a child of v");
        if (c >= nnodes || c == v || parent[c] != parent[v]) return fail(PGM_ERR_INVALID, what + "c is not another child of the parent of v");
    }
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves;
    const size_t nrow = (size_t)nleaves * ncols;

    const size_t mat = (size_t)dim * dim, p_count = mat * nedges;
    const size_t tree_bytes = 4 * tree.size(), pi_off = (tree_bytes + 7) / 8 * 8, w_off = pi_off + 8 * (size_t)dim, par_off = w_off + 8 * (size_t)ncat;
    const size_t cand_off = par_off + 4 * (size_t)nnodes, rows_off = cand_off + 12 * (size_t)ncand;
    const size_t u_count = (size_t)ninner * ncols * dim;
    const size_t cl_count = (size_t)ncat * ncols, ck_bytes = (4 * cl_count + 7) / 8 * 8;   // (L_c, k_c) of every category
    const size_t l_bytes = 8 * (size_t)ncols, k_bytes = (4 * (size_t)ncols + 7) / 8 * 8, rho_bytes = 8 * (size_t)ncand * ncols;
    StageCall c(ctx, "tree nni", &ctx->treelik_ms);
    uint8_t *d_tree = nullptr, *d_g = nullptr, *d_out = nullptr; double *d_P = nullptr, *d_U = nullptr;
    c.buf(pgm_ctx::SC_TREELIK_TREE, rows_off + nrow, &d_tree);
    c.buf(pgm_ctx::SC_TREELIK_P, 8 * p_count * ncat, &d_P);
    c.buf(pgm_ctx::SC_TREELIK_U, 8 * u_count * ncat * 2, &d_U);   // the partials, then the outside vectors
    c.buf(pgm_ctx::SC_TREELIK_G, 8 * cl_count + ck_bytes, &d_g);
    c.buf(pgm_ctx::SC_TREELIK_OUT, l_bytes + k_bytes + 8 * cl_count + rho_bytes, &d_out);
    c.up(d_tree, tree.data(), tree_bytes);
    c.up(d_tree + pi_off, pi, 8 * (size_t)dim);
    c.up(d_tree + w_off, w, 8 * (size_t)ncat);
    c.up(d_tree + par_off, parent, 4 * (size_t)nnodes);
    c.up(d_tree + cand_off, cand_v, 4 * (size_t)ncand);
    c.up(d_tree + cand_off + 4 * (size_t)ncand, cand_a, 4 * (size_t)ncand);
    c.up(d_tree + cand_off + 8 * (size_t)ncand, cand_c, 4 * (size_t)ncand);
    c.up(d_tree + rows_off, rows, nrow);
    c.up(d_P, P, 8 * p_count * ncat);

    PgmTreelikArgs a;
    a.dim = dim; a.nleaves = nleaves; a.nnodes = nnodes; a.ncols = ncols; a.spb = PGM_TREELIK_THREADS / dim; a.derivs = 0;
    a.child_off = (const uint32_t *)d_tree; a.child = a.child_off + nnodes + 1;
    a.pi = (const double *)(d_tree + pi_off); a.rows = (const int8_t *)(d_tree + rows_off); a.P = d_P;
    a.U = d_U; a.O = d_U + u_count * ncat;
    a.g = nullptr; a.h = nullptr;
    a.site_l = (double *)d_g; a.site_k = (int32_t *)(d_g + 8 * cl_count);
    const PgmTreelikRatesStride st = {p_count, u_count, 0, (size_t)ncols};
    PgmTreelikCombineArgs m;
    m.ncat = ncat; m.ncols = ncols; m.nedges = 0;
    m.w = (const double *)(d_tree + w_off); m.L = a.site_l; m.k = a.site_k; m.gc = nullptr; m.qc = nullptr;
    m.site_l = (double *)d_out; m.site_k = (int32_t *)(d_out + l_bytes); m.post = (double *)(d_out + l_bytes + k_bytes);
    m.g = nullptr; m.h = nullptr;
    PgmTreelikNniArgs x;
    x.t = a; x.st = st; x.ncat = ncat; x.ncand = ncand;
    x.parent = (const uint32_t *)(d_tree + par_off);
    x.cand_v = (const uint32_t *)(d_tree + cand_off); x.cand_a = x.cand_v + ncand; x.cand_c = x.cand_a + ncand;
    x.post = m.post; x.rho = m.post + cl_count;
    const uint32_t per = a.spb * PGM_TREELIK_NNI_WAVES;   // sites per workgroup of the candidates' kernel
    const uint32_t blocks = (uint32_t)(((uint64_t)ncols + a.spb - 1) / a.spb), cblocks = (uint32_t)(((uint64_t)ncols + PGM_TREELIK_THREADS - 1) / PGM_TREELIK_THREADS);
    const uint32_t xblocks = (uint32_t)(((uint64_t)ncols + per - 1) / per);
    if (c.begin()) {
        hipLaunchKernelGGL(pgm_treelik_nni_walk_kernel, dim3(blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, c.s, a, st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, c.s, m);
        hipLaunchKernelGGL(pgm_treelik_nni_kernel, dim3(xblocks, std::min<uint32_t>(ncand, 65535u)), dim3(PGM_TREELIK_NNI_THREADS), 0, c.s, x);   // (the kernel strides over the rest)
    }
    c.end();
    c.down(site_l, m.site_l, l_bytes);
    c.down(site_k, m.site_k, 4 * (size_t)ncols);
    c.down(post, m.post, 8 * cl_count);
    c.down(rho, x.rho, rho_bytes);
    return c.finish();
}
