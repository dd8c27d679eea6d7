// pgm_dist_capi.inc — C ABI of the distance-estimation stages (included by pgm_capi.hip).  Every entry is its argument checks, its
// list of device buffers (Buf, in the slots SC_DIST..), the argument struct of its kernel and the launch.
namespace {
// a StageCall whose buffers are one list: staged, `launch` timed into ctx->ml_ms, the results copied back
template <class Launch>
int dist_run(pgm_ctx *ctx, const char *what, std::initializer_list<Buf> bufs, const Launch &launch) {
    StageCall c(ctx, what, &ctx->ml_ms);
    c.bufs(pgm_ctx::SC_DIST, pgm_ctx::SC_DIST_END, bufs);
    for (const Buf &b : bufs) if (b.zero) c.zero(*b.p, b.bytes);
    if (c.begin()) launch(c.s);
    c.end();
    for (const Buf &b : bufs) if (b.dst) c.down(b.dst, *b.p, b.bytes);
    return c.finish();
}
}  // namespace

extern "C" int pgm_mldist_batch(pgm_ctx *ctx, const pgm_mldist_model *m, uint32_t npairs, const int32_t *counts, const uint32_t *gaps,
                                const double *seqlen, double *dist, double *var) {
    // two forms of the model: the eigen form (V, Vi, sigma all given, dim <= 20) and the general form (none of them given, dim <= 64)
    const bool eigen = m && m->V && m->Vi && m->sigma, general = m && !m->V && !m->Vi && !m->sigma;
    if (!ctx || !m || !m->Q || m->dim == 0 || !((eigen && m->dim <= PGM_ML_DMAX) || (general && m->dim <= PGM_MLG_DMAX)))
        return fail(PGM_ERR_INVALID, "bad model (eigen form: Q, V, Vi, sigma and dim <= 20; general form: Q alone, V == Vi == sigma == NULL, and dim <= 64)");
    if (npairs && (!counts || !gaps || !seqlen || !dist || !var)) return fail(PGM_ERR_INVALID, "null argument");
    ctx->ml_ms = 0;
    if (npairs == 0) return PGM_OK;
    const size_t nn = (size_t)m->dim * m->dim;
    double *d_Q = nullptr, *d_V = nullptr, *d_Vi = nullptr, *d_sig = nullptr, *d_len = nullptr, *d_dist = nullptr, *d_var = nullptr;
    int32_t *d_counts = nullptr;
    uint32_t *d_gaps = nullptr;
    return dist_run(ctx, "mldist",
                    {{(void **)&d_Q, 8 * nn, m->Q}, {(void **)&d_V, eigen ? 8 * nn : 0, m->V}, {(void **)&d_Vi, eigen ? 8 * nn : 0, m->Vi},
                     {(void **)&d_sig, eigen ? 8 * (size_t)m->dim : 0, m->sigma}, {(void **)&d_counts, 4 * nn * npairs, counts},
                     {(void **)&d_gaps, 4 * (size_t)npairs, gaps}, {(void **)&d_len, 8 * (size_t)npairs, seqlen},
                     {(void **)&d_dist, 8 * (size_t)npairs, nullptr, dist}, {(void **)&d_var, 8 * (size_t)npairs, nullptr, var}},
                    [&](hipStream_t s) {
        PgmMlArgs A;
        A.dim = m->dim; A.npairs = npairs; A.Q = d_Q; A.V = d_V; A.Vi = d_Vi; A.sigma = d_sig;
        A.counts = d_counts; A.gaps = d_gaps; A.seqlen = d_len;
        A.dist_max = m->dist_max; A.var_max = m->var_max; A.var_min = m->var_min; A.cutoff_dist = m->cutoff_dist;
        A.min_dist = m->min_dist; A.max_dist = m->max_dist; A.indel_rate = m->indel_rate; A.mldist = m->mldist; A.mldist_gap = m->mldist_gap;
        A.dist = d_dist; A.var = d_var;
        const uint32_t blocks = std::min<uint32_t>((npairs + PGM_ML_WAVES - 1) / PGM_ML_WAVES, (uint32_t)ctx->prop.multiProcessorCount * 2u);
        if (eigen) hipLaunchKernelGGL(pgm_mldist_kernel, dim3(blocks), dim3(PGM_ML_WAVES * 64), 0, s, A);
        else hipLaunchKernelGGL(pgm_mldist_general_kernel, dim3(npairs), dim3(PGM_MLG_THREADS), 0, s, A);   // one workgroup per pair
    });
}

extern "C" int pgm_prealigned_counts_batch(pgm_ctx *ctx, uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t npairs,
                                           const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps) {
    if (!ctx || dim < 20 || dim > 64 || (npairs && (!rows || !pi || !pj || !counts || !gaps))) return fail(PGM_ERR_INVALID, "bad argument");
    ctx->ml_ms = 0;
    if (npairs == 0) return PGM_OK;
    for (uint32_t p = 0; p < npairs; ++p)
        if (pi[p] >= nrows || pj[p] >= nrows) return fail(PGM_ERR_INVALID, "pair index out of range");
    int8_t *d_rows = nullptr;
    uint32_t *d_pi = nullptr, *d_pj = nullptr, *d_gaps = nullptr;
    int32_t *d_counts = nullptr;
    return dist_run(ctx, "prealigned",
                    {{(void **)&d_rows, (size_t)nrows * ncols, rows}, {(void **)&d_pi, 4 * (size_t)npairs, pi}, {(void **)&d_pj, 4 * (size_t)npairs, pj},
                     {(void **)&d_counts, 4 * (size_t)npairs * dim * dim, nullptr, counts, true}, {(void **)&d_gaps, 4 * (size_t)npairs, nullptr, gaps}},
                    [&](hipStream_t s) {
        PgmPaArgs A;
        A.dim = dim; A.nrows = nrows; A.ncols = ncols; A.npairs = npairs; A.rows = d_rows; A.pi = d_pi; A.pj = d_pj; A.counts = d_counts; A.gaps = d_gaps;
        const uint32_t blocks = std::min<uint32_t>((npairs + 3) / 4, (uint32_t)ctx->prop.multiProcessorCount * 8u);
        hipLaunchKernelGGL(pgm_prealigned_kernel, dim3(blocks), dim3(256), 0, s, A);
    });
}

extern "C" float pgm_dist_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->ml_ms : 0.f; }

// depth block of the reference's GEMM: L1d / 128 terms, L1d as Eigen reads it from cpuid where the reference runs (48 KB on the
// host of the golden files; PGM_EIGEN_L1D = bytes for another)
static uint32_t kmer_depth_block() {
    const char *l1e = getenv("PGM_EIGEN_L1D");
    const long l1d = l1e ? atol(l1e) : 49152;
    return (uint32_t)std::max(1L, l1d / 128);
}

extern "C" int pgm_kmer_cosine(pgm_ctx *ctx, uint32_t nseq, uint32_t ncols, const int32_t *counts, double *cosine) {
    if (!ctx || (nseq && (!counts || !cosine)) || ncols == 0) return fail(PGM_ERR_INVALID, "bad argument");
    ctx->ml_ms = 0;
    if (nseq == 0) return PGM_OK;
    int32_t *d_counts = nullptr;
    double *d_inv = nullptr, *d_out = nullptr;
    return dist_run(ctx, "kmer cosine",
                    {{(void **)&d_counts, 4 * (size_t)nseq * ncols, counts}, {(void **)&d_inv, 8 * (size_t)nseq}, {(void **)&d_out, 8 * (size_t)nseq * nseq, nullptr, cosine}},
                    [&](hipStream_t s) {
        hipLaunchKernelGGL(pgm_kmer_norm_kernel, dim3((nseq + 255) / 256), dim3(256), 0, s, nseq, ncols, d_counts, d_inv);
        const uint32_t tiles = (nseq + PGM_KC_TILE - 1) / PGM_KC_TILE;
        const uint32_t kc = kmer_depth_block();
        hipLaunchKernelGGL(pgm_kmer_cosine_kernel, dim3(tiles, tiles), dim3(PGM_KC_TILE * PGM_KC_TILE), 0, s, nseq, ncols, d_counts, d_inv, d_out, kc);
    });
}

// ---- many families per launch (pgmsa --batch) ----
extern "C" int pgm_kmer_cosine_multi(pgm_ctx *ctx, uint32_t nfam, const uint32_t *nseq, uint32_t ncols, const int32_t *counts, double *cosine) {
    if (!ctx || !nseq || !counts || !cosine || nfam == 0 || ncols == 0) return fail(PGM_ERR_INVALID, "bad argument");
    ctx->ml_ms = 0;
    std::vector<uint32_t> tile0(nfam + 1, 0), row0(nfam + 1, 0);
    std::vector<uint64_t> out0(nfam + 1, 0);
    for (uint32_t f = 0; f < nfam; ++f) {
        if (nseq[f] < 2) return fail(PGM_ERR_INVALID, "a family needs at least 2 sequences");
        const uint64_t tiles = (nseq[f] + PGM_KC_TILE - 1) / PGM_KC_TILE;
        const uint64_t t = (uint64_t)tile0[f] + tiles * tiles, r = (uint64_t)row0[f] + nseq[f];
        if (t > 0x7fffffffull || r > 0x7fffffffull) return fail(PGM_ERR_INVALID, "too many sequences for one call");
        tile0[f + 1] = (uint32_t)t; row0[f + 1] = (uint32_t)r;
        out0[f + 1] = out0[f] + (uint64_t)nseq[f] * nseq[f];
    }
    const uint32_t nrows = row0[nfam];
    int32_t *d_counts = nullptr;
    double *d_inv = nullptr, *d_out = nullptr;
    uint32_t *d_tile0 = nullptr, *d_row0 = nullptr;
    uint64_t *d_out0 = nullptr;
    return dist_run(ctx, "kmer cosine (multi)",
                    {{(void **)&d_counts, 4 * (size_t)nrows * ncols, counts}, {(void **)&d_inv, 8 * (size_t)nrows}, {(void **)&d_out, 8 * (size_t)out0[nfam], nullptr, cosine},
                     {(void **)&d_tile0, 4 * (size_t)(nfam + 1), tile0.data()}, {(void **)&d_row0, 4 * (size_t)(nfam + 1), row0.data()},
                     {(void **)&d_out0, 8 * (size_t)(nfam + 1), out0.data()}},
                    [&](hipStream_t s) {
        hipLaunchKernelGGL(pgm_kmer_norm_kernel, dim3((nrows + 255) / 256), dim3(256), 0, s, nrows, ncols, d_counts, d_inv);   // (every row has ncols counts)
        hipLaunchKernelGGL(pgm_kmer_cosine_multi_kernel, dim3(tile0[nfam]), dim3(PGM_KC_TILE * PGM_KC_TILE), 0, s, nfam, d_tile0, d_row0, d_out0, ncols, d_counts,
                           d_inv, d_out, kmer_depth_block());
    });
}

extern "C" int pgm_prealigned_counts_multi(pgm_ctx *ctx, uint32_t dim, uint32_t nfam, const uint32_t *nrows, const uint32_t *ncols, const int8_t *rows,
                                           uint32_t npairs, const uint32_t *fam, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps) {
    if (!ctx || dim == 0 || dim > 64 || nfam == 0 || !nrows || !ncols || !rows || !fam || !pi || !pj || !counts || !gaps) return fail(PGM_ERR_INVALID, "bad argument");
    ctx->ml_ms = 0;
    std::vector<uint64_t> base(nfam + 1, 0);
    for (uint32_t f = 0; f < nfam; ++f) {
        if (nrows[f] < 2) return fail(PGM_ERR_INVALID, "a family needs at least 2 rows");
        base[f + 1] = base[f] + (uint64_t)nrows[f] * ncols[f];
    }
    for (uint32_t p = 0; p < npairs; ++p) {
        if (fam[p] >= nfam) return fail(PGM_ERR_INVALID, "family index out of range");
        if (pi[p] >= nrows[fam[p]] || pj[p] >= nrows[fam[p]]) return fail(PGM_ERR_INVALID, "pair index out of range");
    }
    if (npairs == 0) return PGM_OK;
    int8_t *d_rows = nullptr;
    uint64_t *d_base = nullptr;
    uint32_t *d_ncols = nullptr, *d_fam = nullptr, *d_pi = nullptr, *d_pj = nullptr, *d_gaps = nullptr;
    int32_t *d_counts = nullptr;
    return dist_run(ctx, "prealigned (multi)",
                    {{(void **)&d_rows, (size_t)base[nfam], rows}, {(void **)&d_pi, 4 * (size_t)npairs, pi}, {(void **)&d_pj, 4 * (size_t)npairs, pj},
                     {(void **)&d_counts, 4 * (size_t)npairs * dim * dim, nullptr, counts, true}, {(void **)&d_gaps, 4 * (size_t)npairs, nullptr, gaps},
                     {(void **)&d_fam, 4 * (size_t)npairs, fam}, {(void **)&d_base, 8 * (size_t)nfam, base.data()}, {(void **)&d_ncols, 4 * (size_t)nfam, ncols}},
                    [&](hipStream_t s) {
        PgmPaMultiArgs A;
        A.dim = dim; A.npairs = npairs; A.rows = d_rows; A.base = d_base; A.ncols = d_ncols; A.fam = d_fam; A.pi = d_pi; A.pj = d_pj; A.counts = d_counts; A.gaps = d_gaps;
        const uint32_t blocks = std::min<uint32_t>((npairs + 3) / 4, (uint32_t)ctx->prop.multiProcessorCount * 8u);
        hipLaunchKernelGGL(pgm_prealigned_multi_kernel, dim3(blocks), dim3(256), 0, s, A);
    });
}

// ---- resampled columns of one alignment (pgmsa --bootstrap) ----
extern "C" int pgm_prealigned_counts_resampled(pgm_ctx *ctx, uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t nrep,
                                               const uint32_t *cols, uint32_t npairs, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps) {
    if (!ctx || !rows || !cols || !pi || !pj || !counts || !gaps || nrep == 0 || nrows < 2 || ncols == 0 || dim == 0 || dim > 64) return fail(PGM_ERR_INVALID, "bad argument");
    ctx->ml_ms = 0;
    for (uint32_t p = 0; p < npairs; ++p)
        if (pi[p] >= nrows || pj[p] >= nrows) return fail(PGM_ERR_INVALID, "pair index out of range");
    const size_t ncells = (size_t)nrep * ncols;
    for (size_t k = 0; k < ncells; ++k)
        if (cols[k] >= ncols) return fail(PGM_ERR_INVALID, "column index out of range");
    if (npairs == 0) return PGM_OK;
    int8_t *d_rows = nullptr;
    uint32_t *d_pi = nullptr, *d_pj = nullptr, *d_gaps = nullptr, *d_cols = nullptr;
    int32_t *d_counts = nullptr;
    const size_t nout = (size_t)nrep * npairs;
    return dist_run(ctx, "prealigned (resampled)",
                    {{(void **)&d_rows, (size_t)nrows * ncols, rows}, {(void **)&d_pi, 4 * (size_t)npairs, pi}, {(void **)&d_pj, 4 * (size_t)npairs, pj},
                     {(void **)&d_counts, 4 * nout * dim * dim, nullptr, counts, true}, {(void **)&d_gaps, 4 * nout, nullptr, gaps}, {(void **)&d_cols, 4 * ncells, cols}},
                    [&](hipStream_t s) {
        PgmPaResampledArgs A;
        A.dim = dim; A.ncols = ncols; A.npairs = npairs; A.nrep = nrep; A.rows = d_rows; A.cols = d_cols; A.pi = d_pi; A.pj = d_pj; A.counts = d_counts; A.gaps = d_gaps;
        const uint32_t blocks = std::min<uint32_t>((npairs + 3) / 4, (uint32_t)ctx->prop.multiProcessorCount * 8u);
        hipLaunchKernelGGL(pgm_prealigned_resampled_kernel, dim3(blocks, std::min<uint32_t>(nrep, 65535u)), dim3(256), 0, s, A);
    });
}
