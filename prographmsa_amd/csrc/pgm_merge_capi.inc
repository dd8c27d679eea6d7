// pgm_merge_capi.inc — C ABI of the merged-graph node profiles (included by pgm_capi.hip).
static bool merge_is_device(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice;
}

extern "C" int pgm_merge_profiles_batch_ex(pgm_ctx *ctx, uint32_t njobs, const pgm_merge_job *jobs, uint32_t flags, const double **dev_profiles);
extern "C" int pgm_merge_profiles_batch(pgm_ctx *ctx, uint32_t njobs, const pgm_merge_job *jobs) {
    return pgm_merge_profiles_batch_ex(ctx, njobs, jobs, 0u, nullptr);
}

// flags & PGM_MERGE_RESIDENT: the profile matrices stay in HBM (dev_profiles[i] = device address of job i's dim x nnodes doubles,
// valid until pgm_resident_reset on this context) and nothing is copied back; sites1 / sites2 may be such addresses.
extern "C" int pgm_merge_profiles_batch_ex(pgm_ctx *ctx, uint32_t njobs, const pgm_merge_job *jobs, uint32_t flags, const double **dev_profiles) {
    const bool resident = (flags & PGM_MERGE_RESIDENT) != 0;
    if (!ctx || (njobs && !jobs) || (flags & ~PGM_MERGE_RESIDENT) || (resident && njobs && !dev_profiles)) return fail(PGM_ERR_INVALID, "null argument");
    ctx->merge_ms = 0;
    if (njobs == 0) return PGM_OK;
    StageCall c(ctx, "merge", &ctx->merge_ms);   // (the device is current from here on: merge_is_device)
    if (!c.ok()) return c.finish();
    const uint32_t D = jobs[0].dim;
    if (D == 0 || D > 64) return fail(PGM_ERR_INVALID, "bad dimension");
    const int DP = D <= 32 ? 32 : 64, NB = 256 / DP;
    // one host staging image (pinned) -> one H2D copy; outputs come back in one D2H copy
    size_t in_bytes = 0, out_bytes = 0;
    auto al = [](size_t x) { return (x + 15) / 16 * 16; };
    std::vector<char> dev1(njobs, 0), dev2(njobs, 0);   // a child's profiles already are in HBM (left there by a resident call)
    for (uint32_t i = 0; i < njobs; ++i) {
        const pgm_merge_job &j = jobs[i];
        if (j.dim != D || !j.sites1 || !j.sites2 || !j.P1 || !j.P2 || (j.nnodes && (!j.k1 || !j.k2 || !j.g2_with_P1 || (!j.profiles && !resident))))
            return fail(PGM_ERR_INVALID, "invalid merge job " + std::to_string(i));
        dev1[i] = merge_is_device(j.sites1) ? 1 : 0; dev2[i] = merge_is_device(j.sites2) ? 1 : 0;
        for (uint32_t v = 0; v < j.nnodes; ++v)
            if ((j.k1[v] != PGM_GAP && j.k1[v] >= j.n1) || (j.k2[v] != PGM_GAP && j.k2[v] >= j.n2) || (j.k1[v] == PGM_GAP && j.k2[v] == PGM_GAP))
                return fail(PGM_ERR_INVALID, "merge job " + std::to_string(i) + ": bad node mapping");
        in_bytes += (dev1[i] ? 0 : al(8 * (size_t)D * j.n1)) + (dev2[i] ? 0 : al(8 * (size_t)D * j.n2)) + 2 * al(8 * (size_t)D * D) + 2 * al(4 * (size_t)j.nnodes) + al(j.nnodes);
        out_bytes += al(8 * (size_t)D * j.nnodes);
    }
    in_bytes += al(sizeof(PgmMergeJobDev) * njobs);
    // The input image goes through the buffers the alignGraphs batch of the same guide-tree level has just given back to the
    // context's cache (pinned staging + device input: the same graphs' profiles, a little more than that batch uploaded), so a
    // level costs no allocation of its own; they return to the cache at the end.
    uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
    size_t cap_hin = 0, cap_in = 0;
    const bool mprof = getenv("PGM_HOST_PROFILE") != nullptr;   // tools: where the time of the call goes
    auto now_ms = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tm0 = now_ms();
    // (given back when the call is over: behind finish(), which every return below goes through)
    struct GiveBack {
        pgm_ctx *c; uint8_t **h, **d; size_t *ch, *cd;
        ~GiveBack() { cache_give(c, pgm_ctx::C_HIN, *h, *ch); cache_give(c, pgm_ctx::C_IN, *d, *cd); }
    } give_back{ctx, &h_in, &d_in, &cap_hin, &cap_in};
    c.alloc(cache_take(ctx, pgm_ctx::C_HIN, in_bytes, (void **)&h_in, &cap_hin));
    if (c.ok()) c.alloc(cache_take(ctx, pgm_ctx::C_IN, in_bytes, (void **)&d_in, &cap_in));
    if (resident) c.resident(out_bytes, &d_out);   // (valid until pgm_resident_reset)
    else { c.host(pgm_ctx::SH_PROFILES_OUT, out_bytes, &h_out); c.buf(pgm_ctx::SC_MERGE_OUT, out_bytes, &d_out); }
    if (!c.ok()) return c.finish();
    const double tm1 = now_ms();
    std::vector<PgmMergeJobDev> dj(njobs);
    size_t off = al(sizeof(PgmMergeJobDev) * njobs), ooff = 0;
    uint32_t blocks = 0;
    struct Copy { size_t dst; const void *src; size_t bytes; };
    std::vector<Copy> copies;
    copies.reserve(7 * (size_t)njobs);
    auto put = [&](const void *src, size_t bytes) { copies.push_back(Copy{off, src, bytes}); const size_t o = off; off += al(bytes); return o; };
    std::vector<size_t> out_off(njobs);
    for (uint32_t i = 0; i < njobs; ++i) {
        const pgm_merge_job &j = jobs[i];
        PgmMergeJobDev &d = dj[i];
        d.dim = D; d.nnodes = j.nnodes;
        d.sites1 = dev1[i] ? j.sites1 : (const double *)(d_in + put(j.sites1, 8 * (size_t)D * j.n1));
        d.sites2 = dev2[i] ? j.sites2 : (const double *)(d_in + put(j.sites2, 8 * (size_t)D * j.n2));
        d.P1 = (const double *)(d_in + put(j.P1, 8 * (size_t)D * D));
        d.P2 = (const double *)(d_in + put(j.P2, 8 * (size_t)D * D));
        d.k1 = (const uint32_t *)(d_in + put(j.k1, 4 * (size_t)j.nnodes));
        d.k2 = (const uint32_t *)(d_in + put(j.k2, 4 * (size_t)j.nnodes));
        d.g2p1 = (const uint8_t *)(d_in + put(j.g2_with_P1, j.nnodes));
        d.profiles = (double *)(d_out + ooff);
        out_off[i] = ooff;
        ooff += al(8 * (size_t)D * j.nnodes);
        d.first_block = blocks;
        blocks += (j.nnodes + NB - 1) / NB;
    }
    memcpy(h_in, dj.data(), sizeof(PgmMergeJobDev) * njobs);
    {   // the copies into the staging image on a few host threads (a 1024-leaf level is 100 MB of profiles)
        (void)lib_pool().run(copies.size(), in_bytes > (8u << 20) ? 16u : 1u, [&](size_t k) { memcpy(h_in + copies[k].dst, copies[k].src, copies[k].bytes); });
    }
    const double tm2 = now_ms();
    c.up(d_in, h_in, in_bytes);
    if (blocks && c.begin()) {
        const size_t lds = 8 * (2 * (size_t)D * D + 3 * (size_t)NB * D + NB);
        if (DP == 32) hipLaunchKernelGGL((pgm_merge_profiles_kernel<32>), dim3(blocks), dim3(256), lds, c.s, (const PgmMergeJobDev *)d_in, njobs);
        else hipLaunchKernelGGL((pgm_merge_profiles_kernel<64>), dim3(blocks), dim3(256), lds, c.s, (const PgmMergeJobDev *)d_in, njobs);
    }
    if (blocks) c.end();
    if (!resident) c.down(h_out, d_out, out_bytes);
    if (int rc = c.finish()) return rc;
    const double tm3 = now_ms();
    if (resident) {
        for (uint32_t i = 0; i < njobs; ++i) dev_profiles[i] = (const double *)(d_out + out_off[i]);
    } else {   // ... and out of the pinned block into the callers' vectors, on the same few threads
        (void)lib_pool().run(njobs, out_bytes > (8u << 20) ? 16u : 1u, [&](size_t i) { memcpy(jobs[i].profiles, h_out + out_off[i], 8 * (size_t)D * jobs[i].nnodes); });
    }
    if (mprof)
        fprintf(stderr, "    merge: buffers %.2f ms, staging of %.1f MB %.2f, upload + kernel (%.2f) + download of %.1f MB %.2f, copy-out %.2f\n",
                tm1 - tm0, in_bytes / 1e6, tm2 - tm1, ctx->merge_ms, out_bytes / 1e6, tm3 - tm2, now_ms() - tm3);
    return PGM_OK;
}

extern "C" float pgm_merge_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->merge_ms : 0.f; }

// Forget every resident result of the context (the memory is kept for the next ones): the start of a progressive pass.
extern "C" int pgm_resident_reset(pgm_ctx *ctx) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->res_chunk = 0; ctx->res_off = 0;
    return PGM_OK;
}

// A resident matrix of src_ctx copied into ctx's resident memory (see include/pgm_hip.h).  Synchronous.
extern "C" int pgm_resident_import(pgm_ctx *ctx, pgm_ctx *src_ctx, const double *src, uint64_t count, const double **dst) {
    if (!ctx || !src_ctx || !dst || (count && !src)) return fail(PGM_ERR_INVALID, "bad argument");
    *dst = nullptr;
    if (count == 0) return PGM_OK;
    bool known = false;   // the source must lie in src_ctx's resident chunks
    for (const pgm_ctx::ResChunk &c : src_ctx->res_chunks)
        if ((const uint8_t *)src >= c.p && (const uint8_t *)(src + count) <= c.p + c.cap) known = true;
    if (!known) return fail(PGM_ERR_INVALID, "pgm_resident_import: not a resident address of the source context");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = 8 * (size_t)count;
    uint8_t *d_out = nullptr;
    hipError_t e = resident_alloc(ctx, bytes, &d_out);
    if (e == hipSuccess) e = ctx->device == src_ctx->device ? hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, ctx->stream)
                                                            : hipMemcpyPeerAsync(d_out, ctx->device, src, src_ctx->device, bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PGM_ERR_NOMEM : PGM_ERR_DEVICE, std::string("resident import: ") + hipGetErrorString(e));
    *dst = (const double *)d_out;
    return PGM_OK;
}

// Resident leaf graphs: the one-hot profile matrices of nseq sequences, built in HBM (syms: ALPHABET::value(), negative for a residue
// without a value; offs[nseq + 1]); dev[s] = device address of sequence s's dim x (L + 2) matrix, valid until pgm_resident_reset.
extern "C" int pgm_resident_onehot(pgm_ctx *ctx, uint32_t dim, uint32_t nseq, const int8_t *syms, const uint32_t *offs, const double **dev) {
    if (!ctx || dim == 0 || dim > 64 || (nseq && (!syms || !offs || !dev))) return fail(PGM_ERR_INVALID, "bad argument");
    if (nseq == 0) return PGM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const bool prof = getenv("PGM_HOST_PROFILE") != nullptr;
    auto now_ms = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now_ms();
    double t1 = t0, t2 = t0, t3 = t0;
    std::vector<uint64_t> col0(nseq + 1, 0);
    for (uint32_t s = 0; s < nseq; ++s) {
        if (offs[s + 1] < offs[s]) return fail(PGM_ERR_INVALID, "offsets not ascending");
        col0[s + 1] = col0[s] + (offs[s + 1] - offs[s]) + 2;
    }
    for (size_t i = 0; i < offs[nseq]; ++i) if (syms[i] >= (int)dim) return fail(PGM_ERR_INVALID, "symbol out of range");
    const uint64_t ncols = col0[nseq];
    const size_t out_bytes = 8 * (size_t)dim * ncols, nsym = offs[nseq];
    const size_t o_offs = (nsym + 15) & ~(size_t)15, o_col0 = o_offs + ((4 * (size_t)(nseq + 1) + 15) & ~(size_t)15), in_bytes = o_col0 + 8 * (size_t)(nseq + 1);
    // (the 1 + 8 / nseq bytes per residue of input go through a pageable block — a pinned scratch block of their own cost 0.6 ms
    // in the first call of a process, twice the copy and the kernel — and sit behind the matrices in the arena)
    std::vector<uint8_t> staging(in_bytes);
    uint8_t *h_in = staging.data(), *d_in = nullptr, *d_out = nullptr;
    t1 = now_ms();
    t2 = now_ms();
    hipError_t e = resident_alloc(ctx, (out_bytes + 255) / 256 * 256 + in_bytes, &d_out);
    d_in = d_out + (out_bytes + 255) / 256 * 256;
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PGM_ERR_NOMEM : PGM_ERR_DEVICE, std::string("resident leaves: ") + hipGetErrorString(e));
    t3 = now_ms();
    memcpy(h_in, syms, nsym);
    memcpy(h_in + o_offs, offs, 4 * (size_t)(nseq + 1));
    memcpy(h_in + o_col0, col0.data(), 8 * (size_t)(nseq + 1));
    hipStream_t s = ctx->stream;
    e = hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgm_onehot_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, dim, nseq, (const int8_t *)d_in, (const uint32_t *)(d_in + o_offs),
                           (const uint64_t *)(d_in + o_col0), (double *)d_out, ncols);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(PGM_ERR_DEVICE, std::string("resident leaves: ") + hipGetErrorString(e));
    for (uint32_t q = 0; q < nseq; ++q) dev[q] = (const double *)d_out + (size_t)dim * col0[q];
    if (prof) fprintf(stderr, "    resident leaves: checks %.2f ms, scratch buffers %.2f, chunk of the resident arena %.2f, copy + kernel (%.1f MB written) + wait %.2f\n", t1 - t0, t2 - t1, t3 - t2, out_bytes / 1e6, now_ms() - t3);
    return PGM_OK;
}
