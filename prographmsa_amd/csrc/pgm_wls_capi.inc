// pgm_wls_capi.inc — C ABI of the weighted least-squares refinement's subtree pair sums (included by pgm_capi.hip).
// The matrices stay on the device between calls; a call uploads its jobs' labels and offsets in one copy (HostImage),
// runs the two kernels of pgm_wls_kernels.h once per chunk of jobs and copies the sums back.
extern "C" float pgm_wls_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->wls_ms : 0.0f; }
extern "C" uint32_t pgm_wls_last_launches(pgm_ctx *ctx) { return ctx ? ctx->wls_launches : 0u; }

extern "C" int pgm_wls_load(pgm_ctx *ctx, uint32_t n, const double *D, const double *W) {
    if (!ctx || !D || !W) return fail(PGM_ERR_INVALID, "null argument");
    if (n < 2 || n > PGM_WLS_MAX_N) return fail(PGM_ERR_INVALID, "wls: n = " + std::to_string(n) + " outside [2, " + std::to_string(PGM_WLS_MAX_N) + "]");
    ctx->wls_n = 0;
    const size_t nn = (size_t)n * n;
    std::vector<double> dw(2 * nn);
    for (size_t i = 0; i < nn; ++i) { dw[2 * i] = D[i]; dw[2 * i + 1] = W[i]; }
    StageCall c(ctx, "wls matrices", nullptr);
    void *d = nullptr;
    c.buf(pgm_ctx::SC_WLS_MAT, 16 * nn, &d);
    c.up(d, dw.data(), 16 * nn);
    if (int rc = c.finish()) return rc;
    ctx->wls_n = n;
    return PGM_OK;
}

extern "C" int pgm_wls_pair_sums_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_wls_job *jobs, double *out) {
    if (!ctx || (njobs && (!jobs || !out))) return fail(PGM_ERR_INVALID, "null argument");
    ctx->wls_ms = 0;
    ctx->wls_launches = 0;
    const uint32_t n = ctx->wls_n;
    if (n == 0) return fail(PGM_ERR_INVALID, "wls: no matrices loaded (pgm_wls_load)");
    if (njobs == 0) return PGM_OK;
    HostImage img;
    std::vector<PgmWlsJobDev> dj(njobs);
    std::vector<size_t> lab_off(njobs), off_off(njobs);
    img.put(nullptr, sizeof(PgmWlsJobDev) * njobs);
    for (uint32_t i = 0; i < njobs; ++i) {
        const pgm_wls_job &j = jobs[i];
        const std::string what = "wls job " + std::to_string(i) + ": ";
        if (!j.label || !j.offset) return fail(PGM_ERR_INVALID, what + "null pointer");
        if (j.nsub != 4 && j.nsub != 5) return fail(PGM_ERR_INVALID, what + "nsub must be 4 or 5");
        for (uint32_t l = 0; l < n; ++l)
            if (j.label[l] < -1 || j.label[l] >= (int)j.nsub) return fail(PGM_ERR_INVALID, what + "label out of range");
        lab_off[i] = img.put(j.label, n);
        off_off[i] = img.put(j.offset, 8 * (size_t)n);
        dj[i].nsub = j.nsub;
    }
    // jobs per launch: the block partials of a chunk within 64 MB
    const uint32_t nblocks = (n + PGM_WLS_ROWS - 1) / PGM_WLS_ROWS;
    const size_t part_job = (size_t)nblocks * PGM_WLS_SLOTS * 8;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(njobs, (64ull << 20) / part_job));
    StageCall c(ctx, "wls pair sums", &ctx->wls_ms);
    uint8_t *d_in = nullptr; double *d_part = nullptr, *d_out = nullptr;
    c.buf(pgm_ctx::SC_WLS_IN, img.bytes.size(), &d_in);
    c.buf(pgm_ctx::SC_WLS_PART, part_job * chunk, &d_part);
    c.buf(pgm_ctx::SC_WLS_OUT, 8 * PGM_WLS_SLOTS * (size_t)njobs, &d_out);
    for (uint32_t i = 0; i < njobs; ++i) {
        dj[i].label = (const int8_t *)(d_in + lab_off[i]);
        dj[i].offset = (const double *)(d_in + off_off[i]);
    }
    memcpy(img.bytes.data(), dj.data(), sizeof(PgmWlsJobDev) * njobs);
    const double2 *d_mat = (const double2 *)ctx->sc_dev[pgm_ctx::SC_WLS_MAT];
    c.up(d_in, img.bytes.data(), img.bytes.size());
    uint32_t launches = 0;
    if (c.begin())
        for (uint32_t j0 = 0; j0 < njobs; j0 += chunk) {
            const uint32_t nj = std::min(chunk, njobs - j0);
            hipLaunchKernelGGL(pgm_wls_rows_kernel, dim3(nblocks * nj), dim3(256), 0, c.s, d_mat, n, (const PgmWlsJobDev *)d_in + j0, nblocks, d_part);
            hipLaunchKernelGGL(pgm_wls_jobs_kernel, dim3(nj), dim3(64), 0, c.s, (const double *)d_part, nblocks, d_out + (size_t)PGM_WLS_SLOTS * j0);
            launches += 2;
        }
    c.end();
    c.down(out, d_out, 8 * PGM_WLS_SLOTS * (size_t)njobs);
    if (int rc = c.finish()) return rc;
    ctx->wls_launches = launches;
    return PGM_OK;
}
