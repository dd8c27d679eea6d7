// pgm_treelik_rates_capi.inc — C ABI of the tree likelihood under rate categories, pgmsa --ml_tree --ml_gamma (included by
// pgm_capi.hip behind pgm_treelik_capi.inc, whose checks and scratch slots it shares; DESIGN.md 3.18).
// One upload of the tree, the rows, pi, the weights and the matrices of every category; one launch of pgm_treelik_rates_kernel over
// (site block x category), one of pgm_treelik_combine_kernel, with derivs one of pgm_treelik_sums_kernel; one copy back.
extern "C" int pgm_tree_likelihood_rates(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                         const double *pi, uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post,
                                         double *d1, double *d2) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || (derivs && (!d1 || !d2))) return fail(PGM_ERR_INVALID, "null argument");
    if (ncat < 1 || ncat > PGM_TREELIK_MAXCAT) return fail(PGM_ERR_INVALID, "tree likelihood: ncat must be 1 .. " + std::to_string(PGM_TREELIK_MAXCAT));
    for (uint32_t c = 0; c < ncat; ++c)
        if (!(w[c] > 0.0 && w[c] < INFINITY)) return fail(PGM_ERR_INVALID, "tree likelihood: weight " + std::to_string(c) + " is not finite and above 0");
    std::vector<uint32_t> tree;   // child_off, then child
    if (const int rc = treelik_tree(dim, nleaves, nnodes, parent, ncols, rows, tree)) return rc;
    const uint32_t nedges = nnodes - 1, ninner = nnodes - nleaves;
    const size_t nrow = (size_t)nleaves * ncols;

    const size_t mat = (size_t)dim * dim, p_count = mat * (derivs ? 3 : 1) * nedges;
    const size_t tree_bytes = 4 * tree.size(), pi_off = (tree_bytes + 7) / 8 * 8, w_off = pi_off + 8 * (size_t)dim, rows_off = w_off + 8 * (size_t)ncat;
    const size_t u_count = (size_t)ninner * ncols * dim, nchunks = ((size_t)ncols + PGM_TREELIK_CHUNK - 1) / PGM_TREELIK_CHUNK;
    const size_t g_count = derivs ? (size_t)nedges * ncols : 0, part_count = derivs ? 2 * (size_t)nedges * nchunks : 0;
    const size_t cl_count = (size_t)ncat * ncols, ck_bytes = (4 * cl_count + 7) / 8 * 8;   // (L_c, k_c) of every category
    const size_t l_bytes = 8 * (size_t)ncols, k_bytes = (4 * (size_t)ncols + 7) / 8 * 8, d_bytes = 8 * (size_t)nedges;
    StageCall c(ctx, "tree likelihood", &ctx->treelik_ms);
    uint8_t *d_tree = nullptr, *d_g = nullptr, *d_out = nullptr; double *d_P = nullptr, *d_U = nullptr;
    c.buf(pgm_ctx::SC_TREELIK_TREE, rows_off + nrow, &d_tree);
    c.buf(pgm_ctx::SC_TREELIK_P, 8 * p_count * ncat, &d_P);
    c.buf(pgm_ctx::SC_TREELIK_U, 8 * u_count * ncat * (derivs ? 2 : 1), &d_U);
    // (L_c), (k_c), then with derivs (g_c), (q_c) of every category, g, h and the chunk sums
    c.buf(pgm_ctx::SC_TREELIK_G, 8 * cl_count + ck_bytes + 8 * (2 * g_count * ncat + 2 * g_count + part_count), &d_g);
    c.buf(pgm_ctx::SC_TREELIK_OUT, l_bytes + k_bytes + 8 * cl_count + 2 * d_bytes, &d_out);
    c.up(d_tree, tree.data(), tree_bytes);
    c.up(d_tree + pi_off, pi, 8 * (size_t)dim);
    c.up(d_tree + w_off, w, 8 * (size_t)ncat);
    c.up(d_tree + rows_off, rows, nrow);
    c.up(d_P, P, 8 * p_count * ncat);

    double *d_gc = (double *)(d_g + 8 * cl_count + ck_bytes), *d_qc = d_gc + g_count * ncat, *d_gm = d_qc + g_count * ncat, *d_hm = d_gm + g_count;
    PgmTreelikArgs a;
    a.dim = dim; a.nleaves = nleaves; a.nnodes = nnodes; a.ncols = ncols; a.spb = PGM_TREELIK_THREADS / dim; a.derivs = derivs ? 1 : 0;
    a.child_off = (const uint32_t *)d_tree; a.child = a.child_off + nnodes + 1;
    a.pi = (const double *)(d_tree + pi_off); a.rows = (const int8_t *)(d_tree + rows_off); a.P = d_P;
    a.U = d_U; a.O = derivs ? d_U + u_count * ncat : nullptr;
    a.g = derivs ? d_gc : nullptr; a.h = derivs ? d_qc : nullptr;
    a.site_l = (double *)d_g; a.site_k = (int32_t *)(d_g + 8 * cl_count);
    const PgmTreelikRatesStride st = {p_count, u_count, g_count, (size_t)ncols};
    PgmTreelikCombineArgs m;
    m.ncat = ncat; m.ncols = ncols; m.nedges = derivs ? nedges : 0;
    m.w = (const double *)(d_tree + w_off); m.L = a.site_l; m.k = a.site_k; m.gc = d_gc; m.qc = d_qc;
    m.site_l = (double *)d_out; m.site_k = (int32_t *)(d_out + l_bytes); m.post = (double *)(d_out + l_bytes + k_bytes);
    m.g = d_gm; m.h = d_hm;
    double *d_d1 = m.post + cl_count, *d_d2 = d_d1 + nedges;
    const uint32_t blocks = (uint32_t)(((uint64_t)ncols + a.spb - 1) / a.spb), cblocks = (uint32_t)(((uint64_t)ncols + PGM_TREELIK_THREADS - 1) / PGM_TREELIK_THREADS);
    if (c.begin()) {
        hipLaunchKernelGGL(pgm_treelik_rates_kernel, dim3(blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, c.s, a, st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(cblocks, derivs ? std::min<uint32_t>(nedges, 65535u) : 1u), dim3(PGM_TREELIK_THREADS), 0, c.s, m);
        if (derivs)
            hipLaunchKernelGGL(pgm_treelik_sums_kernel, dim3(nedges), dim3(PGM_TREELIK_THREADS), 0, c.s, (const double *)d_gm, (const double *)d_hm, ncols, (uint32_t)nchunks,
                               d_hm + g_count, d_d1, d_d2);
    }
    c.end();
    c.down(site_l, m.site_l, l_bytes);
    c.down(site_k, m.site_k, 4 * (size_t)ncols);
    c.down(post, m.post, 8 * cl_count);
    if (derivs) {
        c.down(d1, d_d1, d_bytes);
        c.down(d2, d_d2, d_bytes);
    }
    return c.finish();
}
