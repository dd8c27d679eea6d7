// pgm_agreement_capi.inc — C ABI of the residue-pair agreement counts of pgmsa --guidance (included by pgm_capi.hip).
// One upload of `where`, the two kernels of pgm_agreement_kernels.h on the zeroed outputs, one copy back of each.
extern "C" float pgm_agreement_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->agree_ms : 0.0f; }

extern "C" int pgm_msa_agreement(pgm_ctx *ctx, uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where, uint32_t *res_hits,
                                 uint32_t *pair_hits) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->agree_ms = 0;
    if (nrows == 0 || ncols == 0 || nrep == 0) return fail(PGM_ERR_INVALID, "msa agreement: nrows, ncols and nrep must be at least 1");
    // the sums are 32-bit: res_hits <= nrep * (nrows - 1), pair_hits <= nrep * ncols (also the pair kernel's chunk index)
    if ((uint64_t)nrep * (nrows - 1) > 0xffffffffull || (uint64_t)nrep * ncols > 0xffffffffull)
        return fail(PGM_ERR_INVALID, "msa agreement: nrep * (nrows - 1) = " + std::to_string((uint64_t)nrep * (nrows - 1)) + " or nrep * ncols = " +
                                         std::to_string((uint64_t)nrep * ncols) + " does not fit 32 bits");
    const uint64_t ntile = ((uint64_t)nrows + PGM_AGREE_T - 1) / PGM_AGREE_T, ctiles = ((uint64_t)ncols + PGM_AGREE_T - 1) / PGM_AGREE_T;
    const uint64_t npair_tiles = ntile * (ntile + 1) / 2, nres_tiles = ntile * ctiles;
    if (npair_tiles > 0x7fffffffull || nres_tiles > 0x7fffffffull) return fail(PGM_ERR_INVALID, "msa agreement: more than 2^31 - 1 tiles in one call");
    if (!where || !res_hits || !pair_hits) return fail(PGM_ERR_INVALID, "null argument");
    const size_t in_bytes = sizeof(int32_t) * (size_t)nrep * nrows * ncols;
    const size_t res_bytes = sizeof(uint32_t) * (size_t)nrows * ncols, pair_bytes = sizeof(uint32_t) * (size_t)nrows * nrows;
    StageCall c(ctx, "msa agreement", &ctx->agree_ms);
    int32_t *d_where = nullptr; uint8_t *d_out = nullptr;
    c.buf(pgm_ctx::SC_AGREE_IN, in_bytes, &d_where);
    c.buf(pgm_ctx::SC_AGREE_OUT, res_bytes + pair_bytes, &d_out);
    uint32_t *d_res = (uint32_t *)d_out, *d_pair = (uint32_t *)(d_out + res_bytes);
    c.up(d_where, where, in_bytes);
    c.zero(d_out, res_bytes + pair_bytes);
    // workgroups per tile along the reduced axis: about four workgroups per CU in all, never more than there are chunks / replicates
    const uint64_t want = 4ull * (uint64_t)std::max(1, ctx->prop.multiProcessorCount);
    const uint64_t nchunks = (uint64_t)nrep * (((uint64_t)ncols + PGM_AGREE_K - 1) / PGM_AGREE_K);
    const uint32_t psplit = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(nchunks, 65535), (want + npair_tiles - 1) / npair_tiles));
    const uint32_t rsplit = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(nrep, 65535), (want + nres_tiles - 1) / nres_tiles));
    if (c.begin()) {
        hipLaunchKernelGGL(pgm_agreement_pairs_kernel, dim3((uint32_t)npair_tiles, psplit), dim3(256), 0, c.s, (const int32_t *)d_where, nrows, ncols, nrep,
                           (uint32_t)ntile, d_pair);
        hipLaunchKernelGGL(pgm_agreement_residues_kernel, dim3((uint32_t)nres_tiles, rsplit), dim3(256), 0, c.s, (const int32_t *)d_where, nrows, ncols, nrep,
                           (uint32_t)ctiles, d_res);
    }
    c.end();
    c.down(res_hits, d_res, res_bytes);
    c.down(pair_hits, d_pair, pair_bytes);
    return c.finish();
}
