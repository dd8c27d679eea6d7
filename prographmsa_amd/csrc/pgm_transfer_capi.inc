// pgm_transfer_capi.inc — C ABI of the transfer indices of pgmsa --bootstrap_tbe (included by pgm_capi.hip).
// The arguments are checked on the host, then: one upload of the reference sets, the replicate offsets and the replicate sets, one
// launch of pgm_transfer_min_kernel<false>, one copy back of phi.  pgm_transfer_taxa_capi.inc has the entry of --bootstrap_taxa.
extern "C" float pgm_transfer_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->transfer_ms : 0.0f; }

// the argument checks both entries share (include/pgm_hip.h: pgm_transfer_min); `what` opens the message
static int transfer_check(const char *what, uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off,
                          const uint64_t *rep, const void *out) {
    const std::string w = std::string(what) + ": ";
    if (nleaves < 4 || nref == 0 || nrep == 0) return fail(PGM_ERR_INVALID, w + "nleaves must be at least 4, nref and nrep at least 1");
    if ((uint64_t)nref * nrep > 0xffffffffull)
        return fail(PGM_ERR_INVALID, w + "nref * nrep = " + std::to_string((uint64_t)nref * nrep) + " does not fit 32 bits");
    if (!ref || !rep_off || !out) return fail(PGM_ERR_INVALID, "null argument");
    if (rep_off[0] != 0) return fail(PGM_ERR_INVALID, w + "rep_off[0] must be 0");
    for (uint32_t r = 0; r < nrep; ++r)
        if (rep_off[r + 1] < rep_off[r]) return fail(PGM_ERR_INVALID, w + "rep_off must ascend (replicate " + std::to_string(r) + ")");
    const size_t nsets = rep_off[nrep];
    if (!rep && nsets != 0) return fail(PGM_ERR_INVALID, "null argument");
    const size_t words = ((size_t)nleaves + 63) / 64;
    const uint64_t tail = nleaves % 64 ? ~(uint64_t)0 << (nleaves % 64) : 0;   // the bits of the last word no leaf has
    for (size_t e = 0; e < nref; ++e) {
        size_t size = 0;
        for (size_t k = 0; k < words; ++k) size += (size_t)__builtin_popcountll(ref[e * words + k]);
        if (ref[e * words + words - 1] & tail) return fail(PGM_ERR_INVALID, w + "reference set " + std::to_string(e) + " has a bit at or above nleaves");
        if (size == 0 || size == nleaves) return fail(PGM_ERR_INVALID, w + "reference set " + std::to_string(e) + " is empty or full");
    }
    for (size_t s = 0; s < nsets; ++s)
        if (rep[s * words + words - 1] & tail) return fail(PGM_ERR_INVALID, w + "replicate set " + std::to_string(s) + " has a bit at or above nleaves");
    return PGM_OK;
}

extern "C" int pgm_transfer_min(pgm_ctx *ctx, uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off,
                                const uint64_t *rep, uint32_t *phi) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->transfer_ms = 0;
    if (int rc = transfer_check("transfer min", nleaves, nref, ref, nrep, rep_off, rep, phi)) return rc;
    const size_t nsets = rep_off[nrep], words = ((size_t)nleaves + 63) / 64;

    const size_t ref_bytes = 8 * words * (size_t)nref, off_bytes = sizeof(uint32_t) * ((size_t)nrep + 1), rep_bytes = 8 * words * nsets;
    const size_t phi_bytes = sizeof(uint32_t) * (size_t)nref * nrep;
    StageCall c(ctx, "transfer min", &ctx->transfer_ms);
    uint8_t *d_ref = nullptr; uint64_t *d_rep = nullptr; uint32_t *d_phi = nullptr;
    c.buf(pgm_ctx::SC_TRANSFER_REF, ref_bytes + off_bytes, &d_ref);
    c.buf(pgm_ctx::SC_TRANSFER_REP, rep_bytes, &d_rep);
    c.buf(pgm_ctx::SC_TRANSFER_OUT, phi_bytes, &d_phi);
    uint32_t *d_off = (uint32_t *)(d_ref + ref_bytes);
    c.up(d_ref, ref, ref_bytes);
    c.up(d_off, rep_off, off_bytes);
    c.up(d_rep, rep, rep_bytes);
    const uint32_t tiles = (uint32_t)(((uint64_t)nref + PGM_TRANSFER_T - 1) / PGM_TRANSFER_T);
    // a workgroup per (reference tile, replicate); beyond the grid's y range a workgroup takes several replicates in turn
    if (c.begin())
        hipLaunchKernelGGL(pgm_transfer_min_kernel<false>, dim3(tiles, std::min<uint32_t>(nrep, 65535)), dim3(256), 0, c.s, (const uint32_t *)d_ref, nref,
                           (const uint32_t *)d_rep, (const uint32_t *)d_off, nrep, nleaves, (uint32_t)(2 * words), d_phi, (uint32_t *)nullptr, (uint32_t *)nullptr);
    c.end();
    c.down(phi, d_phi, phi_bytes);
    return c.finish();
}
