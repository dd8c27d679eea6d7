// pgm_csprofile_capi.inc — C ABI of the context-specific profile stage (included by pgm_capi.hip).
extern "C" int pgm_csprofile_load(pgm_ctx *ctx, uint32_t K, uint32_t ncols, const double *lprofiles, const double *centre,
                                  const double *priors) {
    if (!ctx || !K || !ncols || ncols > 31 || !lprofiles || !centre || !priors) return fail(PGM_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->cs_lprofiles) { (void)hipFree(ctx->cs_lprofiles); ctx->cs_lprofiles = nullptr; }
    if (ctx->cs_centre) { (void)hipFree(ctx->cs_centre); ctx->cs_centre = nullptr; }
    if (ctx->cs_priors) { (void)hipFree(ctx->cs_priors); ctx->cs_priors = nullptr; }
    // device format: one record per profile (see pgm_csprofile_kernel)
    const size_t rec = ((size_t)ncols + 1) * 22;
    std::vector<double> lib((size_t)K * rec, 0.0);
    for (uint32_t k = 0; k < K; ++k) {
        double *r = lib.data() + (size_t)k * rec;
        for (uint32_t c = 0; c < ncols; ++c)
            for (uint32_t e = 0; e < 21; ++e) r[c * 22 + e] = lprofiles[((size_t)k * ncols + c) * 21 + e];
        for (uint32_t a = 0; a < 20; ++a) r[(size_t)ncols * 22 + a] = centre[(size_t)k * 20 + a];
        r[(size_t)ncols * 22 + 20] = priors[k];
    }
    HIPCHK(hipMalloc((void **)&ctx->cs_lprofiles, 8 * lib.size()));
    HIPCHK(hipMemcpy(ctx->cs_lprofiles, lib.data(), 8 * lib.size(), hipMemcpyHostToDevice));
    ctx->csK = K;
    ctx->csC = ncols;
    return PGM_OK;
}

// (dev != NULL: the profile matrices stay in the context's resident arena — pgm_csprofile_create_batch_res —, dev[s] = the 20 x (len + 2)
// matrix of sequence s; `out` / `out_offs` are not used then)
static int csprofile_create_batch_impl(pgm_ctx *ctx, uint32_t nseq, const int8_t *syms, const uint32_t *offs,
                                       const double *tau, const double *pi, const double *p_uniform, double *out,
                                       const uint64_t *out_offs, const double **dev) {
    if (!ctx || !ctx->csK) return fail(PGM_ERR_INVALID, "no profile library loaded");
    if (nseq && (!syms || !offs || !tau || !pi || !p_uniform || (!dev && (!out || !out_offs)))) return fail(PGM_ERR_INVALID, "null argument");
    ctx->cs_ms = 0;
    if (nseq == 0) return PGM_OK;
    std::vector<uint64_t> own_offs;
    if (dev) {
        own_offs.assign((size_t)nseq + 1, 0);
        for (uint32_t s = 0; s < nseq; ++s) {
            if (offs[s + 1] < offs[s]) return fail(PGM_ERR_INVALID, "offsets not ascending");
            own_offs[s + 1] = own_offs[s] + (uint64_t)20 * (offs[s + 1] - offs[s] + 2);
        }
        out_offs = own_offs.data();
    }
    const uint32_t total = offs[nseq];
    for (uint32_t i = 0; i < total; ++i)
        if (syms[i] < 0 || syms[i] > 20) return fail(PGM_ERR_INVALID, "symbol out of range");
    std::vector<uint32_t> pos_seq(std::max(total, 1u));
    for (uint32_t s = 0; s < nseq; ++s) {
        if (out_offs[s + 1] - out_offs[s] != (uint64_t)20 * (offs[s + 1] - offs[s] + 2)) return fail(PGM_ERR_INVALID, "out_offs mismatch");
        for (uint32_t i = offs[s]; i < offs[s + 1]; ++i) pos_seq[i] = s;
    }
    const size_t out_n = out_offs[nseq];
    int8_t *d_syms = nullptr;
    uint32_t *d_offs = nullptr, *d_pos = nullptr;
    double *d_tau = nullptr, *d_pi = nullptr, *d_pu = nullptr, *d_out = nullptr;
    uint64_t *d_oo = nullptr;
    StageCall c(ctx, "csprofile", &ctx->cs_ms);
    c.bufs(pgm_ctx::SC_CS, pgm_ctx::SC_CS_END,
           {{(void **)&d_syms, std::max(total, 1u), syms}, {(void **)&d_offs, 4 * (size_t)(nseq + 1), offs},
            {(void **)&d_pos, 4 * (size_t)std::max(total, 1u), pos_seq.data()}, {(void **)&d_tau, 8 * (size_t)nseq, tau},
            {(void **)&d_pi, 8 * 20, pi}, {(void **)&d_pu, 8 * (size_t)nseq * 20, p_uniform},
            {(void **)&d_oo, 8 * (size_t)(nseq + 1), out_offs}, {(void **)&d_out, dev ? 16 : 8 * out_n}});
    double *h_out = nullptr;
    if (dev) c.resident(8 * out_n, &d_out);   // the output in the context's resident memory
    else c.host(pgm_ctx::SH_PROFILES_OUT, 8 * out_n, &h_out);
    c.zero(d_out, 8 * out_n);  // sequences of length 0 keep their two zero columns
    if (total && c.begin()) {
        PgmCsArgs A;
        A.K = ctx->csK; A.ncols = ctx->csC; A.nseq = nseq;
        A.lprofiles = ctx->cs_lprofiles;
        A.syms = d_syms; A.offs = d_offs; A.pos_seq = d_pos; A.tau = d_tau; A.pi = d_pi; A.p_uniform = d_pu;
        A.out = d_out; A.out_offs = d_oo; A.total = total;
        const size_t cs_lds = sizeof(double) * PGM_CS_KC * (((size_t)A.ncols + 1) * 22);
        hipLaunchKernelGGL(pgm_csprofile_kernel, dim3((total + 255) / 256), dim3(256), cs_lds, c.s, A);
    }
    if (total) c.end();
    if (!dev) c.down(h_out, d_out, 8 * out_n);
    if (int rc = c.finish()) return rc;
    if (dev) for (uint32_t q = 0; q < nseq; ++q) dev[q] = d_out + out_offs[q];
    else memcpy(out, h_out, 8 * out_n);
    return PGM_OK;
}

extern "C" int pgm_csprofile_create_batch(pgm_ctx *ctx, uint32_t nseq, const int8_t *syms, const uint32_t *offs,
                                          const double *tau, const double *pi, const double *p_uniform, double *out,
                                          const uint64_t *out_offs) {
    return csprofile_create_batch_impl(ctx, nseq, syms, offs, tau, pi, p_uniform, out, out_offs, nullptr);
}
extern "C" int pgm_csprofile_create_batch_res(pgm_ctx *ctx, uint32_t nseq, const int8_t *syms, const uint32_t *offs,
                                              const double *tau, const double *pi, const double *p_uniform, const double **dev) {
    if (nseq && !dev) return fail(PGM_ERR_INVALID, "null argument");
    return csprofile_create_batch_impl(ctx, nseq, syms, offs, tau, pi, p_uniform, nullptr, nullptr, dev);
}

extern "C" float pgm_csprofile_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->cs_ms : 0.f; }
