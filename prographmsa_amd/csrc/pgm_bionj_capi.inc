// pgm_bionj_capi.inc — C ABI of the BioNJ joins (included by pgm_capi.hip).  A call uploads the families' matrices, the family
// descriptors and the identity index lists, runs the three kernels of pgm_bionj_kernels.h once per join of the largest family
// (plain launches on the context's stream: stream order is the only dependency), and copies the join log and final_d back in
// one copy behind one synchronisation.  With a plan of joins (pgm_bionj_plan_multi) the kernels are two launches in all: the
// preparation, then every join of every family.
extern "C" float pgm_bionj_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->bionj_ms : 0.0f; }
extern "C" uint32_t pgm_bionj_last_launches(pgm_ctx *ctx) { return ctx ? ctx->bionj_launches : 0u; }

namespace {
// plan == nullptr: every join's pair is the criterion's first minimum (three kernels per join); else the pairs of `plan`
int bionj_run(pgm_ctx *ctx, uint32_t nfam, const uint32_t *n, const double *D, const double *V, const pgm_bionj_pair *plan,
              pgm_bionj_join *joins, double *final_d) {
    if (ctx) { ctx->bionj_ms = 0; ctx->bionj_launches = 0; }
    if (!ctx || !n || !D || !V || !joins || !final_d) return fail(PGM_ERR_INVALID, "null argument");
    if (nfam == 0) return fail(PGM_ERR_INVALID, "bionj: no family");
    std::vector<PgmBionjFam> fam(nfam);
    uint64_t sum_nn = 0, sum_n = 0, sum_j = 0;
    uint32_t nmax = 0;
    for (uint32_t f = 0; f < nfam; ++f) {
        if (n[f] < 4 || n[f] > PGM_BIONJ_MAX_N)
            return fail(PGM_ERR_INVALID, "bionj: family " + std::to_string(f) + ": n = " + std::to_string(n[f]) + " outside [4, " + std::to_string(PGM_BIONJ_MAX_N) + "]");
        fam[f] = PgmBionjFam{n[f], sum_nn, sum_n, sum_j};
        sum_nn += (uint64_t)n[f] * n[f]; sum_n += n[f]; sum_j += n[f] - 3u;
        nmax = std::max(nmax, n[f]);
    }
    {   // a NaN or an infinity: std::max / std::min of the host loop propagate them in ways the parallel minimum does not
        const uint64_t grain = (uint64_t)1 << 16, nchunks = (sum_nn + grain - 1) / grain;
        std::atomic<int> bad(0);
        (void)lib_pool().run((size_t)nchunks, nchunks >= 16 ? 16u : 1u, [&](size_t c) {
            const uint64_t e0 = c * grain, e1 = std::min<uint64_t>(sum_nn, e0 + grain);
            bool ok = true;
            for (uint64_t e = e0; e < e1; ++e) ok = ok && std::isfinite(D[e]) && std::isfinite(V[e]);
            if (!ok) bad.store(1);
        });
        if (bad.load()) return fail(PGM_ERR_INVALID, "bionj: a distance or variance is not finite");
    }
    if (plan)   // the kernel indexes the matrices with these
        for (uint32_t f = 0; f < nfam; ++f)
            for (uint32_t s = 0; s + 3u < n[f]; ++s) {
                const pgm_bionj_pair &p = plan[fam[f].joff + s];
                if (p.index1 >= p.index2 || p.index2 >= n[f] - s)
                    return fail(PGM_ERR_INVALID, "bionj: family " + std::to_string(f) + ": pair (" + std::to_string(p.index1) + ", " + std::to_string(p.index2) + ") of join " +
                                                     std::to_string(s) + " is not index1 < index2 < " + std::to_string(n[f] - s));
            }
    // the vector buffer: sums, best_q (doubles), the descriptors, act[0], act[1], best_row; descriptors and act[0] are uploaded
    const size_t o_sums = 0, o_bq = o_sums + 8 * sum_n, o_fam = o_bq + 8 * sum_n, o_act0 = o_fam + sizeof(PgmBionjFam) * nfam,
                 o_act1 = o_act0 + 4 * sum_n, o_brow = o_act1 + 4 * sum_n, o_plan = o_brow + 4 * sum_n,
                 vec_bytes = o_plan + (plan ? sizeof(pgm_bionj_pair) * sum_j : 0);   // (the plan behind the rest: uploaded)
    const size_t out_joins = sizeof(pgm_bionj_join) * sum_j, out_bytes = out_joins + 8 * 9 * (size_t)nfam;
    HostImage img(1);   // (the device layout of o_fam .. o_act1: no padding)
    img.put(fam.data(), sizeof(PgmBionjFam) * nfam);
    {
        const size_t o = img.put(nullptr, 4 * sum_n);
        uint32_t *a = (uint32_t *)(img.bytes.data() + o);
        for (uint32_t f = 0; f < nfam; ++f)
            for (uint32_t i = 0; i < n[f]; ++i) a[fam[f].voff + i] = i;
    }
    StageCall c(ctx, "bionj", &ctx->bionj_ms);
    uint8_t *d_mat = nullptr, *d_vec = nullptr, *d_out = nullptr;
    c.buf(pgm_ctx::SC_BIONJ_MAT, 3 * 8 * (size_t)sum_nn, &d_mat);
    c.buf(pgm_ctx::SC_BIONJ_VEC, vec_bytes, &d_vec);
    c.buf(pgm_ctx::SC_BIONJ_OUT, out_bytes, &d_out);
    PgmBionjDev S;
    S.fam = (const PgmBionjFam *)(d_vec + o_fam); S.nfam = nfam;
    S.D = (double *)d_mat; S.T = S.D + sum_nn; S.V = S.T + sum_nn;
    S.act[0] = (uint32_t *)(d_vec + o_act0); S.act[1] = (uint32_t *)(d_vec + o_act1);
    S.sums = (double *)(d_vec + o_sums); S.best_q = (double *)(d_vec + o_bq); S.best_row = (uint32_t *)(d_vec + o_brow);
    S.joins = (pgm_bionj_join *)d_out; S.final_d = (double *)(d_out + out_joins);
    hipStream_t s = c.s;
    c.up(S.D, D, 8 * (size_t)sum_nn);
    c.up(S.V, V, 8 * (size_t)sum_nn);
    c.up(d_vec + o_fam, img.bytes.data(), img.bytes.size());
    if (plan) c.up(d_vec + o_plan, plan, sizeof(pgm_bionj_pair) * sum_j);
    const uint32_t gy = std::min(nfam, 65535u), gz = (nfam + gy - 1) / gy;
    uint32_t launches = 0;
    const bool go = c.begin();
    if (go && plan) {   // the clamp of every matrix, then one workgroup per family for all of its joins
        const uint32_t gx = (uint32_t)std::min<uint64_t>(((uint64_t)nmax * nmax + 255u) / 256u, 1024u);
        hipLaunchKernelGGL(pgm_bionj_prepare_kernel, dim3(gx, gy, gz), dim3(256), 0, s, S);
        hipLaunchKernelGGL(pgm_bionj_plan_kernel, dim3(1, gy, gz), dim3(256), 0, s, S, (const pgm_bionj_pair *)(d_vec + o_plan));
        launches = 2;
    } else {
        for (uint32_t step = 0; go && step + 3u < nmax; ++step) {
            const dim3 cols((nmax - step + PGM_BIONJ_COLS - 1) / PGM_BIONJ_COLS, gy, gz);
            hipLaunchKernelGGL(pgm_bionj_sums_kernel, cols, dim3(64 * PGM_BIONJ_COLS), 0, s, S, step);
            hipLaunchKernelGGL(pgm_bionj_scan_kernel, cols, dim3(64 * PGM_BIONJ_COLS), 0, s, S, step);
            hipLaunchKernelGGL(pgm_bionj_join_kernel, dim3(1, gy, gz), dim3(256), 0, s, S, step);
            launches += 3;
        }
    }
    c.end();
    std::vector<uint8_t> back(out_bytes);
    c.down(back.data(), d_out, out_bytes);
    if (int rc = c.finish()) return rc;
    memcpy(joins, back.data(), out_joins);
    memcpy(final_d, back.data() + out_joins, out_bytes - out_joins);
    ctx->bionj_launches = launches;
    return PGM_OK;
}
}  // namespace

extern "C" int pgm_bionj_multi(pgm_ctx *ctx, uint32_t nfam, const uint32_t *n, const double *D, const double *V,
                               pgm_bionj_join *joins, double *final_d) {
    return bionj_run(ctx, nfam, n, D, V, nullptr, joins, final_d);
}

extern "C" int pgm_bionj_plan_multi(pgm_ctx *ctx, uint32_t nfam, const uint32_t *n, const double *D, const double *V,
                                    const pgm_bionj_pair *plan, pgm_bionj_join *joins, double *final_d) {
    if (!plan) {
        if (ctx) { ctx->bionj_ms = 0; ctx->bionj_launches = 0; }
        return fail(PGM_ERR_INVALID, "null argument");
    }
    return bionj_run(ctx, nfam, n, D, V, plan, joins, final_d);
}

extern "C" int pgm_bionj_plan(pgm_ctx *ctx, uint32_t n, const double *D, const double *V, const pgm_bionj_pair *plan,
                              pgm_bionj_join *joins, double *final_d) {
    return pgm_bionj_plan_multi(ctx, 1, &n, D, V, plan, joins, final_d);
}

extern "C" int pgm_bionj(pgm_ctx *ctx, uint32_t n, const double *D, const double *V, pgm_bionj_join *joins, double *final_d) {
    return pgm_bionj_multi(ctx, 1, &n, D, V, joins, final_d);
}
