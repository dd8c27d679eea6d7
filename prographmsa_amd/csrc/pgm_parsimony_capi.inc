// pgm_parsimony_capi.inc — C ABI of the root search's gap masks and gap parsimony (included by pgm_capi.hip).
// The inputs of a call are packed into one host image, uploaded in one copy, and the outputs come back in one copy.
extern "C" float pgm_parsimony_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->pars_ms : 0.0f; }

extern "C" int pgm_gapmask_extend_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_gapmask_job *jobs) {
    if (!ctx || (njobs && !jobs)) return fail(PGM_ERR_INVALID, "null argument");
    ctx->pars_ms = 0;
    if (njobs == 0) return PGM_OK;
    HostImage img;
    std::vector<PgmGapmaskJobDev> dj(njobs);
    std::vector<size_t> src_off(njobs), rank_off(njobs), dst_off(njobs);
    size_t out_words = 0;
    img.put(nullptr, sizeof(PgmGapmaskJobDev) * njobs);   // (descriptors first: filled in below)
    std::vector<int32_t> rank;
    for (uint32_t i = 0; i < njobs; ++i) {
        const pgm_gapmask_job &j = jobs[i];
        if ((j.nrows && j.ncols_in && !j.src) || (j.ncols_out && !j.mapping) || (j.nrows && j.ncols_out && !j.dst))
            return fail(PGM_ERR_INVALID, "gap mask job " + std::to_string(i) + ": null pointer");
        rank.assign(j.ncols_out, -1);
        uint32_t k = 0;
        for (uint32_t c = 0; c < j.ncols_out; ++c)
            if (j.mapping[c] != PGM_GAP) { if (k == j.ncols_in) break; rank[c] = (int32_t)k++; }
        uint32_t mapped = 0;
        for (uint32_t c = 0; c < j.ncols_out; ++c) mapped += j.mapping[c] != PGM_GAP;
        if (mapped != j.ncols_in) return fail(PGM_ERR_INVALID, "gap mask job " + std::to_string(i) + ": the mapping does not cover the child's columns");
        const uint32_t wi = (j.ncols_in + 63) / 64, wo = (j.ncols_out + 63) / 64;
        src_off[i] = img.put(j.src, 8 * (size_t)j.nrows * wi);
        rank_off[i] = img.put(rank.data(), 4 * (size_t)j.ncols_out);
        dst_off[i] = out_words;
        out_words += (size_t)j.nrows * wo;
        dj[i].nrows = j.nrows; dj[i].words_in = wi; dj[i].ncols_out = j.ncols_out; dj[i].words_out = wo;
    }
    StageCall c(ctx, "gap masks", &ctx->pars_ms);
    uint8_t *d_in = nullptr; uint64_t *d_out = nullptr;
    c.buf(pgm_ctx::SC_PARS_IN, img.bytes.size(), &d_in);
    c.buf(pgm_ctx::SC_PARS_OUT, 8 * out_words, &d_out);
    for (uint32_t i = 0; i < njobs; ++i) {
        dj[i].src = (const uint64_t *)(d_in + src_off[i]);
        dj[i].rank = (const int32_t *)(d_in + rank_off[i]);
        dj[i].dst = d_out + dst_off[i];
    }
    memcpy(img.bytes.data(), dj.data(), sizeof(PgmGapmaskJobDev) * njobs);
    std::vector<uint64_t> out(out_words);
    c.up(d_in, img.bytes.data(), img.bytes.size());
    if (c.begin()) hipLaunchKernelGGL(pgm_gapmask_extend_kernel, dim3(std::min<uint32_t>(njobs, 65535u)), dim3(256), 0, c.s, (const PgmGapmaskJobDev *)d_in, njobs);
    c.end();
    c.down(out.data(), d_out, 8 * out_words);
    if (int rc = c.finish()) return rc;
    for (uint32_t i = 0; i < njobs; ++i)
        if (jobs[i].nrows && jobs[i].ncols_out) memcpy(jobs[i].dst, out.data() + dst_off[i], 8 * (size_t)jobs[i].nrows * dj[i].words_out);
    return PGM_OK;
}

extern "C" int pgm_gap_parsimony_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_parsimony_job *jobs, uint32_t *scores) {
    if (!ctx || (njobs && (!jobs || !scores))) return fail(PGM_ERR_INVALID, "null argument");
    ctx->pars_ms = 0;
    if (njobs == 0) return PGM_OK;
    HostImage img;
    std::vector<PgmParsimonyJobDev> dj(njobs);
    std::vector<size_t> mask_off(njobs), ch_off(njobs);
    uint64_t per_wg = 1;   // scratch words one workgroup needs: (nleaves - 2) internal consensus rows of nblocks words
    img.put(nullptr, sizeof(PgmParsimonyJobDev) * njobs);
    std::vector<uint8_t> seen;
    for (uint32_t i = 0; i < njobs; ++i) {
        const pgm_parsimony_job &j = jobs[i];
        const std::string what = "parsimony job " + std::to_string(i) + ": ";
        if (j.nleaves < 2) return fail(PGM_ERR_INVALID, what + "fewer than two rows");
        if (j.ncols == 0) return fail(PGM_ERR_INVALID, what + "no columns");
        if (!j.masks || !j.children) return fail(PGM_ERR_INVALID, what + "null pointer");
        const uint32_t ninner = j.nleaves - 1;
        seen.assign((size_t)j.nleaves + ninner, 0);
        for (uint32_t k = 0; k < ninner; ++k)
            for (int s = 0; s < 2; ++s) {
                const uint32_t c = j.children[2 * (size_t)k + s];
                if (c >= j.nleaves + k) return fail(PGM_ERR_INVALID, what + "child out of range or not in post-order");
                if (seen[c]++) return fail(PGM_ERR_INVALID, what + "a node is the child of two nodes");
            }
        const uint32_t words = (j.ncols + 63) / 64, nb = (j.ncols + 31) / 32;
        mask_off[i] = img.put(j.masks, 8 * (size_t)j.nleaves * words);
        ch_off[i] = img.put(j.children, 8 * (size_t)ninner);
        dj[i].nleaves = j.nleaves; dj[i].ncols = j.ncols; dj[i].words = words; dj[i].nblocks = nb;
        per_wg = std::max<uint64_t>(per_wg, (uint64_t)(ninner - 1) * nb);
    }
    // one workgroup per candidate, as many at a time as 256 MB of consensus scratch hold
    const uint64_t budget = (256ull << 20) / 8;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)njobs, budget / per_wg, 65535u}));
    StageCall c(ctx, "gap parsimony", &ctx->pars_ms);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    const size_t score_bytes = (4 * (size_t)njobs + 255) / 256 * 256;
    c.buf(pgm_ctx::SC_PARS_IN, img.bytes.size(), &d_in);
    c.buf(pgm_ctx::SC_PARS_OUT, score_bytes + 8 * per_wg * grid, &d_out);
    for (uint32_t i = 0; i < njobs; ++i) {
        dj[i].masks = (const uint64_t *)(d_in + mask_off[i]);
        dj[i].children = (const uint32_t *)(d_in + ch_off[i]);
    }
    memcpy(img.bytes.data(), dj.data(), sizeof(PgmParsimonyJobDev) * njobs);
    c.up(d_in, img.bytes.data(), img.bytes.size());
    if (c.begin())
        hipLaunchKernelGGL(pgm_gap_parsimony_kernel, dim3(grid), dim3(256), 0, c.s, (const PgmParsimonyJobDev *)d_in, njobs,
                           (uint64_t *)(d_out + score_bytes), per_wg, (uint32_t *)d_out);
    c.end();
    c.down(scores, d_out, 4 * (size_t)njobs);
    return c.finish();
}
