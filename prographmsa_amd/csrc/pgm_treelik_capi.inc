// pgm_treelik_capi.inc — C ABI of the tree likelihood and what is built on it (included by pgm_capi.hip): pgm_tree_likelihood
// (pgmsa --ml_tree, DESIGN.md 3.17), pgm_tree_likelihood_rates (--ml_gamma, 3.18), pgm_tree_ancestral (--ml_ancestral, 3.19),
// pgm_tree_nni (--ml_search, 3.20), pgm_tree_nni_edge (--ml_nni_opt, 3.22) and pgm_tree_spr (--ml_spr, 3.23).  The arguments are checked on the host and the children lists are built there
// (pgm_treelik_check.h), then: one upload of the inputs, the launches, one copy back.  pgm_tree_ancestral_joint and
// pgm_tree_ancestral_sample (--ml_ancestral_joint, --ml_ancestral_samples, 3.24) are the last two.  The eight entries share five scratch
// slots, laid out by pgm_treelik_plan.h.  Stateless: nothing of a call is read by the next.
extern "C" float pgm_treelik_last_kernel_ms(pgm_ctx *ctx) { return ctx ? ctx->treelik_ms : 0.0f; }

// What every entry does past its own null checks: the shared refusals (ncat and the weights, the tree, the candidates), the slots,
// the upload of the inputs, and the arguments of the walk (a, st) and of pgm_treelik_combine_kernel (m) from the plan.
struct TreelikIn {
    uint32_t dim, nleaves, nnodes; const uint32_t *parent; uint32_t ncols; const int8_t *rows; const double *pi;
    uint32_t ncat; const double *w, *P; int derivs;   // (ncat, w: all but the plain entry)
    uint32_t ncand; const uint32_t *cand_v, *cand_a, *cand_c; bool full;
    const double *Pc = nullptr;   // (pgm_tree_nni_edge alone)
    const double *Ph = nullptr; const uint32_t *cand_y = nullptr;   // (pgm_tree_spr alone)
    uint32_t nsamp = 0;           // (pgm_tree_ancestral_sample alone)
};
static_assert(pgm_ctx::SC_TREELIK_OUT - pgm_ctx::SC_TREELIK_TREE == PGM_TL_SLOT_OUT, "the five slots in the order of pgm_treelik_plan.h");
struct TreelikCall {
    std::optional<StageCall> c;   // (opened once nothing is refused any more)
    PgmTreelikPlan pl;
    uint8_t *slot[PGM_TL_NSLOTS] = {};
    PgmTreelikArgs a;
    PgmTreelikRatesStride st;
    PgmTreelikCombineArgs m;
    std::vector<uint32_t> path;   // pgm_tree_spr: the candidates' paths (pgm_treelik_check_spr)
    uint32_t blocks, cblocks;     // of the walk (sites / spb) and of the combine kernel (sites / 64)
    template <class T> T *at(int region) const { return pl.r[region].bytes ? (T *)(slot[pl.r[region].slot] + pl.r[region].off) : nullptr; }

    int open(pgm_ctx *ctx, const char *what, int mode, const TreelikIn &in) {
        std::string bad = mode != PGM_TREELIK_CALL_PLAIN ? pgm_treelik_check_rates(in.ncat, in.w) : std::string();
        std::vector<uint32_t> tree;   // child_off, then child
        if (bad.empty()) bad = pgm_treelik_check_tree(in.dim, in.nleaves, in.nnodes, in.parent, in.ncols, in.rows, tree);
        if (bad.empty() && (mode == PGM_TREELIK_CALL_NNI || mode == PGM_TREELIK_CALL_NNI_EDGE)) bad = pgm_treelik_check_candidates(in.nleaves, in.nnodes, in.parent, in.ncand, in.cand_v, in.cand_a, in.cand_c);
        if (bad.empty() && mode == PGM_TREELIK_CALL_SPR) bad = pgm_treelik_check_spr(in.nnodes, in.parent, tree.data(), in.ncand, in.cand_v, in.cand_y, path);
        if (!bad.empty()) return fail(PGM_ERR_INVALID, bad);
        pl = pgm_treelik_plan(mode, in.dim, in.nleaves, in.nnodes, in.ncols, in.ncat, in.derivs != 0, in.ncand, in.full, in.nsamp);
        c.emplace(ctx, what, &ctx->treelik_ms);
        for (int k = 0; k < PGM_TL_NSLOTS; ++k)
            if (pl.slot_bytes[k]) c->buf(pgm_ctx::SC_TREELIK_TREE + k, pl.slot_bytes[k], &slot[k]);
        c->up(at<void>(PGM_TL_CHILD), tree.data(), pl.r[PGM_TL_CHILD].bytes);
        c->up(at<void>(PGM_TL_PI), in.pi, pl.r[PGM_TL_PI].bytes);
        c->up(at<void>(PGM_TL_W), in.w, pl.r[PGM_TL_W].bytes);
        c->up(at<void>(PGM_TL_PARENT), in.parent, pl.r[PGM_TL_PARENT].bytes);
        if (pl.r[PGM_TL_CAND].bytes) {
            c->up(at<uint32_t>(PGM_TL_CAND), in.cand_v, 4 * (size_t)in.ncand);
            c->up(at<uint32_t>(PGM_TL_CAND) + in.ncand, in.cand_a, 4 * (size_t)in.ncand);
            c->up(at<uint32_t>(PGM_TL_CAND) + 2 * (size_t)in.ncand, in.cand_c, 4 * (size_t)in.ncand);
        }
        c->up(at<void>(PGM_TL_ROWS), in.rows, pl.r[PGM_TL_ROWS].bytes);
        c->up(at<void>(PGM_TL_P), in.P, pl.r[PGM_TL_P].bytes);
        c->up(at<void>(PGM_TL_PC), in.Pc, pl.r[PGM_TL_PC].bytes);
        c->up(at<void>(PGM_TL_PH), in.Ph, pl.r[PGM_TL_PH].bytes);
        c->up(at<void>(PGM_TL_SPR_CAND), in.cand_v, pl.r[PGM_TL_SPR_CAND].bytes);   // (cand_y: the last node of a candidate's path)
        c->up(at<void>(PGM_TL_SPR_PATH), path.data(), pl.r[PGM_TL_SPR_PATH].bytes);

        const bool cats = mode != PGM_TREELIK_CALL_PLAIN;   // the walk writes the categories' values; the combine kernel the outputs
        a.dim = in.dim; a.nleaves = in.nleaves; a.nnodes = in.nnodes; a.ncols = in.ncols; a.spb = PGM_TREELIK_THREADS / in.dim; a.derivs = in.derivs ? 1 : 0;
        a.child_off = at<const uint32_t>(PGM_TL_CHILD); a.child = a.child_off + in.nnodes + 1;
        a.pi = at<const double>(PGM_TL_PI); a.rows = at<const int8_t>(PGM_TL_ROWS); a.P = at<const double>(PGM_TL_P);
        a.U = at<double>(PGM_TL_U); a.O = at<double>(PGM_TL_O);
        a.g = at<double>(cats ? PGM_TL_GC : PGM_TL_G); a.h = at<double>(cats ? PGM_TL_QC : PGM_TL_H);
        a.site_l = at<double>(cats ? PGM_TL_CL : PGM_TL_SITE_L); a.site_k = at<int32_t>(cats ? PGM_TL_CK : PGM_TL_SITE_K);
        st = {pl.p_count, pl.u_count, pl.g_count, (size_t)in.ncols};
        m.ncat = in.ncat; m.ncols = in.ncols; m.nedges = in.derivs ? pl.nedges : 0;
        m.w = at<const double>(PGM_TL_W); m.L = a.site_l; m.k = a.site_k; m.gc = a.g; m.qc = a.h;
        m.site_l = at<double>(PGM_TL_SITE_L); m.site_k = at<int32_t>(PGM_TL_SITE_K); m.post = at<double>(PGM_TL_POST);
        m.g = at<double>(PGM_TL_G); m.h = at<double>(PGM_TL_H);
        blocks = (uint32_t)(((uint64_t)in.ncols + a.spb - 1) / a.spb);
        cblocks = (uint32_t)(((uint64_t)in.ncols + PGM_TREELIK_THREADS - 1) / PGM_TREELIK_THREADS);
        return PGM_OK;
    }
    // with derivs: the sums of the per-site ratios into D1 and D2, per edge (pgm_tree_nni_edge: `rows` candidates in their place)
    void launch_sums(uint32_t rows) {
        hipLaunchKernelGGL(pgm_treelik_sums_kernel, dim3(rows), dim3(PGM_TREELIK_THREADS), 0, c->s, at<const double>(PGM_TL_G), at<const double>(PGM_TL_H), a.ncols,
                           (uint32_t)pl.nchunks, at<double>(PGM_TL_PART), at<double>(PGM_TL_D1), at<double>(PGM_TL_D2));
    }
    // the outputs every entry has (post, d1, d2: where the call has them)
    void down(double *site_l, int32_t *site_k, double *post, double *d1, double *d2) {
        c->down(site_l, at<void>(PGM_TL_SITE_L), pl.r[PGM_TL_SITE_L].bytes);
        c->down(site_k, at<void>(PGM_TL_SITE_K), pl.r[PGM_TL_SITE_K].bytes);
        c->down(post, at<void>(PGM_TL_POST), pl.r[PGM_TL_POST].bytes);
        c->down(d1, at<void>(PGM_TL_D1), pl.r[PGM_TL_D1].bytes);
        c->down(d2, at<void>(PGM_TL_D2), pl.r[PGM_TL_D2].bytes);
    }
};

// One launch of pgm_treelik_kernel (a workgroup per block of sites walks the whole tree), with derivs one of pgm_treelik_sums_kernel.
extern "C" int pgm_tree_likelihood(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                   const double *pi, const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !P || !site_l || !site_k || (derivs && (!d1 || !d2))) return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    if (const int rc = t.open(ctx, "tree likelihood", PGM_TREELIK_CALL_PLAIN, {dim, nleaves, nnodes, parent, ncols, rows, pi, 0, nullptr, P, derivs, 0, nullptr, nullptr, nullptr, false}))
        return rc;
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_kernel, dim3(t.blocks), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a);
        if (derivs) t.launch_sums(t.pl.nedges);
    }
    t.c->end();
    t.down(site_l, site_k, nullptr, d1, d2);
    return t.c->finish();
}

// One launch of the walk over (site block x category), one of pgm_treelik_combine_kernel, with derivs one of pgm_treelik_sums_kernel.
extern "C" int pgm_tree_likelihood_rates(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                         const double *pi, uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post,
                                         double *d1, double *d2) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || (derivs && (!d1 || !d2))) return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    if (const int rc = t.open(ctx, "tree likelihood", PGM_TREELIK_CALL_RATES, {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, derivs, 0, nullptr, nullptr, nullptr, false}))
        return rc;
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_RAW>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, derivs ? std::min<uint32_t>(t.pl.nedges, 65535u) : 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        if (derivs) t.launch_sums(t.pl.nedges);
    }
    t.c->end();
    t.down(site_l, site_k, post, d1, d2);
    return t.c->finish();
}

// The walk in its ancestral mode over (site block x category), pgm_treelik_combine_kernel for site_l, site_k and post, then
// pgm_treelik_anc_combine_kernel.  The categories' posteriors stand where pgm_tree_likelihood_rates keeps the outside vectors.
extern "C" int pgm_tree_ancestral(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                  const double *pi, uint32_t ncat, const double *w, const double *P, double *site_l, int32_t *site_k, double *post,
                                  int8_t *anc_state, double *anc_prob, double *anc_post) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || !anc_state || !anc_prob) return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    if (const int rc = t.open(ctx, "tree ancestral", PGM_TREELIK_CALL_ANC, {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, 0, 0, nullptr, nullptr, nullptr, anc_post != nullptr}))
        return rc;
    PgmTreelikAncCombineArgs x;
    x.dim = dim; x.ncat = ncat; x.ncols = ncols; x.spb = t.a.spb; x.npairs = t.pl.npairs; x.cat = t.pl.u_count;
    x.a = t.a.O; x.post = t.m.post;
    x.anc_prob = t.at<double>(PGM_TL_ANC_PROB); x.anc_state = t.at<int8_t>(PGM_TL_ANC_STATE); x.anc_post = t.at<double>(PGM_TL_ANC_POST);
    const uint32_t xblocks = (uint32_t)std::min<uint64_t>(((uint64_t)x.npairs + x.spb - 1) / x.spb, (uint64_t)1 << 20);   // (the kernel strides over the rest)
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_ANC>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        hipLaunchKernelGGL(pgm_treelik_anc_combine_kernel, dim3(xblocks), dim3(PGM_TREELIK_THREADS), 0, t.c->s, x);
    }
    t.c->end();
    t.down(site_l, site_k, post, nullptr, nullptr);
    t.c->down(anc_prob, x.anc_prob, t.pl.r[PGM_TL_ANC_PROB].bytes);
    t.c->down(anc_state, x.anc_state, t.pl.r[PGM_TL_ANC_STATE].bytes);
    t.c->down(anc_post, x.anc_post, t.pl.r[PGM_TL_ANC_POST].bytes);
    return t.c->finish();
}

// The walk in its nni mode over (site block x category), which leaves the partials and the outside vectors in device memory,
// pgm_treelik_combine_kernel for site_l, site_k and post, then pgm_treelik_nni_kernel over (site block x candidate).
extern "C" int pgm_tree_nni(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                            const double *pi, uint32_t ncat, const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a,
                            const uint32_t *cand_c, double *site_l, int32_t *site_k, double *post, double *rho) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || !cand_v || !cand_a || !cand_c || !rho) return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    if (const int rc = t.open(ctx, "tree nni", PGM_TREELIK_CALL_NNI, {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, 0, ncand, cand_v, cand_a, cand_c, false}))
        return rc;
    PgmTreelikNniArgs x;
    x.t = t.a; x.st = t.st; x.ncat = ncat; x.ncand = ncand;
    x.parent = t.at<const uint32_t>(PGM_TL_PARENT);
    x.cand_v = t.at<const uint32_t>(PGM_TL_CAND); x.cand_a = x.cand_v + ncand; x.cand_c = x.cand_a + ncand;
    x.post = t.m.post; x.rho = t.at<double>(PGM_TL_RHO);
    x.Pc = nullptr; x.g = x.h = nullptr;
    const uint32_t per = t.a.spb * PGM_TREELIK_NNI_WAVES;   // sites per workgroup of the candidates' kernel
    const uint32_t xblocks = (uint32_t)(((uint64_t)ncols + per - 1) / per);
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_NNI>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        hipLaunchKernelGGL(pgm_treelik_nni_kernel<false>, dim3(xblocks, std::min<uint32_t>(ncand, 65535u)), dim3(PGM_TREELIK_NNI_THREADS), 0, t.c->s, x);   // (the kernel strides over the rest)
    }
    t.c->end();
    t.down(site_l, site_k, post, nullptr, nullptr);
    t.c->down(rho, x.rho, t.pl.r[PGM_TL_RHO].bytes);
    return t.c->finish();
}

// pgm_tree_nni with the candidates' own matrices of the edge above v: the same walk and combine launches, pgm_treelik_nni_kernel in
// its EDGE form over (site block x candidate), which also writes the per-site g and h of every candidate, then
// pgm_treelik_sums_kernel with the candidates in the place of the edges.
extern "C" int pgm_tree_nni_edge(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                 const double *pi, uint32_t ncat, const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a,
                                 const uint32_t *cand_c, const double *Pc, double *site_l, int32_t *site_k, double *post, double *rho, double *d1, double *d2) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || !cand_v || !cand_a || !cand_c || !rho || !Pc || !d1 || !d2)
        return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    if (const int rc = t.open(ctx, "tree nni edge", PGM_TREELIK_CALL_NNI_EDGE, {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, 0, ncand, cand_v, cand_a, cand_c, false, Pc}))
        return rc;
    PgmTreelikNniArgs x;
    x.t = t.a; x.st = t.st; x.ncat = ncat; x.ncand = ncand;
    x.parent = t.at<const uint32_t>(PGM_TL_PARENT);
    x.cand_v = t.at<const uint32_t>(PGM_TL_CAND); x.cand_a = x.cand_v + ncand; x.cand_c = x.cand_a + ncand;
    x.post = t.m.post; x.rho = t.at<double>(PGM_TL_RHO);
    x.Pc = t.at<const double>(PGM_TL_PC); x.g = t.at<double>(PGM_TL_G); x.h = t.at<double>(PGM_TL_H);
    const uint32_t per = t.a.spb * PGM_TREELIK_NNI_WAVES;
    const uint32_t xblocks = (uint32_t)(((uint64_t)ncols + per - 1) / per);
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_NNI>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        hipLaunchKernelGGL(pgm_treelik_nni_kernel<true>, dim3(xblocks, std::min<uint32_t>(ncand, 65535u)), dim3(PGM_TREELIK_NNI_THREADS), 0, t.c->s, x);   // (the kernel strides over the rest)
        t.launch_sums(ncand);
    }
    t.c->end();
    t.down(site_l, site_k, post, d1, d2);
    t.c->down(rho, x.rho, t.pl.r[PGM_TL_RHO].bytes);
    return t.c->finish();
}

// The same walk and combine launches as pgm_tree_nni, then pgm_treelik_spr_kernel over (site block x candidate): a workgroup recomputes
// the chain of its candidate from the paths pgm_treelik_check_spr wrote, so the order of the candidates changes no value.
extern "C" int pgm_tree_spr(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                            const double *pi, uint32_t ncat, const double *w, const double *P, const double *Ph, uint32_t ncand, const uint32_t *cand_v,
                            const uint32_t *cand_y, double *site_l, int32_t *site_k, double *post, double *rho) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !Ph || !site_l || !site_k || !post || !cand_v || !cand_y || !rho) return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    TreelikIn in = {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, 0, ncand, cand_v, nullptr, nullptr, false};
    in.Ph = Ph; in.cand_y = cand_y;
    if (const int rc = t.open(ctx, "tree spr", PGM_TREELIK_CALL_SPR, in)) return rc;
    PgmTreelikSprArgs x;
    x.t = t.a; x.st = t.st; x.ncat = ncat; x.ncand = ncand; x.stride = PGM_TREELIK_SPR_STRIDE;
    x.cand_v = t.at<const uint32_t>(PGM_TL_SPR_CAND); x.path = t.at<const uint32_t>(PGM_TL_SPR_PATH);
    x.Ph = t.at<const double>(PGM_TL_PH); x.post = t.m.post; x.rho = t.at<double>(PGM_TL_RHO);
    const uint32_t per = t.a.spb * PGM_TREELIK_NNI_WAVES;   // sites per workgroup of the candidates' kernel
    const uint32_t xblocks = (uint32_t)(((uint64_t)ncols + per - 1) / per);
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_NNI>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        hipLaunchKernelGGL(pgm_treelik_spr_kernel, dim3(xblocks, std::min<uint32_t>(ncand, 65535u)), dim3(PGM_TREELIK_NNI_THREADS), 0, t.c->s, x);   // (the kernel strides over the rest)
    }
    t.c->end();
    t.down(site_l, site_k, post, nullptr, nullptr);
    t.c->down(rho, x.rho, t.pl.r[PGM_TL_RHO].bytes);
    return t.c->finish();
}

// The walk and the combine launches of pgm_tree_likelihood_rates without derivs, then pgm_treelik_joint_kernel (the max pass, a
// workgroup per block of sites as in the walk) and pgm_treelik_joint_trace_kernel (a thread per site).
extern "C" int pgm_tree_ancestral_joint(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                        const double *pi, uint32_t ncat, const double *w, const double *P, double *site_l, int32_t *site_k, double *post, uint8_t *cat,
                                        int8_t *joint_state, double *joint_l, int32_t *joint_k) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || !cat || !joint_state || !joint_l || !joint_k) return fail(PGM_ERR_INVALID, "null argument");
    TreelikCall t;
    if (const int rc = t.open(ctx, "tree ancestral joint", PGM_TREELIK_CALL_JOINT, {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, 0, 0, nullptr, nullptr, nullptr, false}))
        return rc;
    PgmTreelikJointArgs x;
    x.t = t.a; x.pstride = t.pl.p_count; x.ncat = ncat;
    x.parent = t.at<const uint32_t>(PGM_TL_PARENT); x.post = t.m.post;
    x.F = t.at<double>(PGM_TL_JF); x.ptr = t.at<uint8_t>(PGM_TL_JPTR);
    x.cat = t.at<uint8_t>(PGM_TL_JCAT); x.state = t.at<int8_t>(PGM_TL_JSTATE); x.joint_l = t.at<double>(PGM_TL_JL); x.joint_k = t.at<int32_t>(PGM_TL_JK);
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_RAW>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        hipLaunchKernelGGL(pgm_treelik_joint_kernel, dim3(t.blocks), dim3(PGM_TREELIK_THREADS), 0, t.c->s, x);
        hipLaunchKernelGGL(pgm_treelik_joint_trace_kernel, dim3(t.cblocks), dim3(PGM_TREELIK_THREADS), 0, t.c->s, x);
    }
    t.c->end();
    t.down(site_l, site_k, post, nullptr, nullptr);
    t.c->down(cat, x.cat, t.pl.r[PGM_TL_JCAT].bytes);
    t.c->down(joint_state, x.state, t.pl.r[PGM_TL_JSTATE].bytes);
    t.c->down(joint_l, x.joint_l, t.pl.r[PGM_TL_JL].bytes);
    t.c->down(joint_k, x.joint_k, t.pl.r[PGM_TL_JK].bytes);
    return t.c->finish();
}

// The same walk and combine launches, then pgm_treelik_sample_kernel over (block of 64 samples x site): a lane is a sample.
extern "C" int pgm_tree_ancestral_sample(pgm_ctx *ctx, uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows,
                                         const double *pi, uint32_t ncat, const double *w, const double *P, uint32_t nsamp, uint64_t first_sample, uint64_t seed,
                                         double *site_l, int32_t *site_k, double *post, uint8_t *samp_cat, int8_t *samp_state) {
    if (!ctx) return fail(PGM_ERR_INVALID, "null argument");
    ctx->treelik_ms = 0;
    if (!parent || !rows || !pi || !w || !P || !site_l || !site_k || !post || !samp_cat || !samp_state) return fail(PGM_ERR_INVALID, "null argument");
    if (nsamp == 0) return fail(PGM_ERR_INVALID, "tree ancestral sample: no sample");
    TreelikCall t;
    TreelikIn in = {dim, nleaves, nnodes, parent, ncols, rows, pi, ncat, w, P, 0, 0, nullptr, nullptr, nullptr, false};
    in.nsamp = nsamp;
    if (const int rc = t.open(ctx, "tree ancestral sample", PGM_TREELIK_CALL_SAMPLE, in)) return rc;
    PgmTreelikSampleArgs x;
    x.t = t.a; x.st = t.st; x.ncat = ncat; x.nsamp = nsamp; x.first = first_sample; x.seed = seed;
    x.parent = t.at<const uint32_t>(PGM_TL_PARENT); x.post = t.m.post;
    x.cat = t.at<uint8_t>(PGM_TL_SCAT); x.state = t.at<int8_t>(PGM_TL_SSTATE);
    const uint32_t sblocks = (nsamp - 1) / PGM_TREELIK_THREADS + 1;
    if (t.c->begin()) {
        hipLaunchKernelGGL(pgm_treelik_cat_kernel<PGM_TREELIK_RAW>, dim3(t.blocks, ncat), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.a, t.st);
        hipLaunchKernelGGL(pgm_treelik_combine_kernel, dim3(t.cblocks, 1u), dim3(PGM_TREELIK_THREADS), 0, t.c->s, t.m);
        hipLaunchKernelGGL(pgm_treelik_sample_kernel, dim3(sblocks, std::min<uint32_t>(ncols, 65535u)), dim3(PGM_TREELIK_THREADS), 0, t.c->s, x);   // (the kernel strides over the rest)
    }
    t.c->end();
    t.down(site_l, site_k, post, nullptr, nullptr);
    t.c->down(samp_cat, x.cat, t.pl.r[PGM_TL_SCAT].bytes);
    t.c->down(samp_state, x.state, t.pl.r[PGM_TL_SSTATE].bytes);
    return t.c->finish();
}
