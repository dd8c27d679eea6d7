// pgm_transfer_taxa_capi.inc — C ABI of the moved-taxon counts of pgmsa --bootstrap_taxa (included by pgm_capi.hip behind
// pgm_transfer_capi.inc, whose checks, scratch slots and timer it shares).  The arguments are checked on the host, then: one upload
// of the reference sets with the replicate offsets and the thresholds, and of the replicate sets; pgm_transfer_min_kernel<true>
// (phi, arg, flip) and pgm_transfer_moved_kernel (moved, counted) on the context's stream; one copy back of each output.
static_assert(PGM_TRANSFER_NOSET == PGM_TRANSFER_NONE, "the kernels write PGM_TRANSFER_NONE of include/pgm_hip.h");

extern "C" int pgm_transfer_taxa(pgm_ctx *ctx, uint32_t nleaves, uint32_t nref, const uint64_t *ref, const uint32_t *thr, uint32_t nrep,
                                 const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi, uint32_t *arg, uint32_t *moved, uint32_t *counted) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->transfer_ms = 0;
    if (!thr || !arg || !moved || !counted) return fail(PGM_ERR_INVALID, "null argument");
    if (nleaves > 0x7fffffffu) return fail(PGM_ERR_INVALID, "transfer taxa: nleaves = " + std::to_string(nleaves) + " is beyond 2^31 - 1");
    if ((uint64_t)nref * nleaves > 0xffffffffull)
        return fail(PGM_ERR_INVALID, "transfer taxa: nref * nleaves = " + std::to_string((uint64_t)nref * nleaves) + " does not fit 32 bits");
    if (int rc = transfer_check("transfer taxa", nleaves, nref, ref, nrep, rep_off, rep, phi)) return rc;
    const size_t nsets = rep_off[nrep], words = ((size_t)nleaves + 63) / 64;

    const size_t ref_bytes = 8 * words * (size_t)nref, off_bytes = sizeof(uint32_t) * ((size_t)nrep + 1), thr_bytes = sizeof(uint32_t) * (size_t)nref;
    const size_t rep_bytes = 8 * words * nsets, phi_bytes = sizeof(uint32_t) * (size_t)nref * nrep, moved_bytes = sizeof(uint32_t) * (size_t)nref * nleaves;
    StageCall c(ctx, "transfer taxa", &ctx->transfer_ms);
    uint8_t *d_ref = nullptr, *d_out = nullptr; uint64_t *d_rep = nullptr;
    c.buf(pgm_ctx::SC_TRANSFER_REF, ref_bytes + off_bytes + thr_bytes, &d_ref);
    c.buf(pgm_ctx::SC_TRANSFER_REP, rep_bytes, &d_rep);
    c.buf(pgm_ctx::SC_TRANSFER_OUT, 3 * phi_bytes + moved_bytes + thr_bytes, &d_out);   // phi, arg, flip, moved, counted
    uint32_t *d_off = (uint32_t *)(d_ref + ref_bytes), *d_thr = (uint32_t *)(d_ref + ref_bytes + off_bytes);
    uint32_t *d_phi = (uint32_t *)d_out, *d_arg = (uint32_t *)(d_out + phi_bytes), *d_flip = (uint32_t *)(d_out + 2 * phi_bytes);
    uint32_t *d_moved = (uint32_t *)(d_out + 3 * phi_bytes), *d_counted = (uint32_t *)(d_out + 3 * phi_bytes + moved_bytes);
    c.up(d_ref, ref, ref_bytes);
    c.up(d_off, rep_off, off_bytes);
    c.up(d_thr, thr, thr_bytes);
    c.up(d_rep, rep, rep_bytes);
    const uint32_t tiles = (uint32_t)(((uint64_t)nref + PGM_TRANSFER_T - 1) / PGM_TRANSFER_T);
    if (c.begin()) {
        hipLaunchKernelGGL(pgm_transfer_min_kernel<true>, dim3(tiles, std::min<uint32_t>(nrep, 65535)), dim3(256), 0, c.s, (const uint32_t *)d_ref, nref,
                           (const uint32_t *)d_rep, (const uint32_t *)d_off, nrep, nleaves, (uint32_t)(2 * words), d_phi, d_arg, d_flip);
        // a workgroup per (reference set, 256 leaves); beyond the grid's y range a workgroup takes several tiles of leaves in turn
        hipLaunchKernelGGL(pgm_transfer_moved_kernel, dim3(nref, std::min<uint32_t>((nleaves + 255) / 256, 65535)), dim3(256), 0, c.s, (const uint32_t *)d_ref,
                           (const uint32_t *)d_rep, nrep, nleaves, (uint32_t)(2 * words), (const uint32_t *)d_thr, (const uint32_t *)d_phi, (const uint32_t *)d_arg,
                           (const uint32_t *)d_flip, d_moved, d_counted);
    }
    c.end();
    c.down(phi, d_phi, phi_bytes);
    c.down(arg, d_arg, phi_bytes);
    c.down(moved, d_moved, moved_bytes);
    c.down(counted, d_counted, thr_bytes);
    return c.finish();
}
