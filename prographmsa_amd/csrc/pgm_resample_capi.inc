// pgm_resample_capi.inc — C ABI of the sums over resampled columns of pgmsa --ml_tree --ml_support (included by pgm_capi.hip;
// DESIGN.md 3.21).  The arguments are checked on the host, then: one upload of x and of cols, one launch of
// pgm_resample_transpose_kernel, one of pgm_resample_sums_kernel, one copy back of out.
extern "C" float pgm_resample_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->resample_ms : 0.0f; }

extern "C" int pgm_resampled_sums(pgm_ctx *ctx, uint32_t nrow, uint32_t ncols, const double *x, uint32_t nrep, const uint32_t *cols, double *out) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->resample_ms = 0;
    if (!x || !cols || !out) return fail(PGM_ERR_INVALID, "null argument");
    if (nrow == 0 || ncols == 0 || nrep == 0) return fail(PGM_ERR_INVALID, "resampled sums: nrow, ncols and nrep must be at least 1");
    if ((uint64_t)nrow * nrep > 0xffffffffull)
        return fail(PGM_ERR_INVALID, "resampled sums: nrow * nrep = " + std::to_string((uint64_t)nrow * nrep) + " does not fit 32 bits");
    if ((uint64_t)nrep * ncols > 0xffffffffull)
        return fail(PGM_ERR_INVALID, "resampled sums: nrep * ncols = " + std::to_string((uint64_t)nrep * ncols) + " does not fit 32 bits");
    const size_t ncol_entries = (size_t)nrep * ncols;
    for (size_t k = 0; k < ncol_entries; ++k)
        if (cols[k] >= ncols)
            return fail(PGM_ERR_INVALID, "resampled sums: replicate " + std::to_string(k / ncols) + " draws column " + std::to_string(cols[k]) + " of " + std::to_string(ncols));

    const size_t pitch = ((size_t)nrow + PGM_RESAMPLE_T - 1) / PGM_RESAMPLE_T * PGM_RESAMPLE_T, qtiles = pitch / PGM_RESAMPLE_T;
    const size_t x_bytes = 8 * (size_t)nrow * ncols, xt_bytes = 8 * pitch * ncols, cols_bytes = 4 * ncol_entries, out_bytes = 8 * (size_t)nrow * nrep;
    StageCall c(ctx, "resampled sums", &ctx->resample_ms);
    double *d_x = nullptr, *d_xt = nullptr, *d_out = nullptr; uint32_t *d_cols = nullptr;
    c.buf(pgm_ctx::SC_RESAMPLE_X, x_bytes, &d_x);
    c.buf(pgm_ctx::SC_RESAMPLE_XT, xt_bytes, &d_xt);
    c.buf(pgm_ctx::SC_RESAMPLE_COLS, cols_bytes, &d_cols);
    c.buf(pgm_ctx::SC_RESAMPLE_OUT, out_bytes, &d_out);
    c.up(d_x, x, x_bytes);
    c.up(d_cols, cols, cols_bytes);
    const uint32_t ngroups = (uint32_t)(((uint64_t)nrep + PGM_RESAMPLE_GROUP - 1) / PGM_RESAMPLE_GROUP);
    const uint64_t nitems = (qtiles + PGM_RESAMPLE_XCDS - 1) / PGM_RESAMPLE_XCDS * PGM_RESAMPLE_XCDS * (uint64_t)ngroups;
    if (c.begin()) {
        hipLaunchKernelGGL(pgm_resample_transpose_kernel, dim3((uint32_t)(((uint64_t)ncols + 31) / 32),(uint32_t)std::min<size_t>(pitch / 32, 65535)), dim3(256), 0, c.s, d_x, nrow, ncols, pitch,
                           d_xt);   // (the kernel strides over the rest)
        hipLaunchKernelGGL(pgm_resample_sums_kernel, dim3((uint32_t)std::min<uint64_t>(nitems, PGM_RESAMPLE_MAXGRID)), dim3(64 * PGM_RESAMPLE_WAVES), 0, c.s, d_xt, nrow, ncols,
                           pitch, nrep, d_cols, nitems, ngroups, d_out);
    }
    c.end();
    c.down(out, d_out, out_bytes);
    return c.finish();
}
