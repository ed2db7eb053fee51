// abi_pressure.inc -- C ABI: pressure chambers (kernels_pressure.hpp, pressure.hpp) and the load admm_hip_step adds before its prologue
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  The load writes v and nothing else of the solver's state; it runs eagerly on the context's
// stream, outside the captured iteration and frame graphs, and drops none of them.  A context with no chamber, or whose chambers are
// all inactive, launches nothing here.

static admm_dev::PresDev pres_dev(const admm_hip_ctx *ctx) {
    admm_dev::PresDev d{};
    d.blocks = (const admm_dev::PresBlock *)ctx->d_pres_blk; d.chambers = (const admm_dev::PresChamber *)ctx->d_pres_chm; d.law = (const admm_dev::PresLaw *)ctx->d_pres_law;
    d.tri = ctx->d_pres_tri; d.tri_chamber = ctx->d_pres_trichm; d.rec = (admm_pressure::Record *)ctx->d_pres_rec; d.collapsed = ctx->d_pres_collapsed;
    d.nrm = ctx->d_pres_nrm; d.part = ctx->d_pres_part; d.n_blocks_total = ctx->pres_blocks; d.n_tris_total = ctx->pres_tris;
    d.node = ctx->d_pres_node; d.ptr = ctx->d_pres_ptr; d.off = ctx->d_pres_off; d.stride = ctx->d_pres_stride; d.n_nodes = ctx->pres_nodes;
    return d;
}

static int pres_check_law(admm_hip_ctx *ctx, const char *who, int chamber, int mode, const double *params) {
    if (mode != ADMM_PRESSURE_CONSTANT && mode != ADMM_PRESSURE_GAS) return fail(ctx, ADMM_ERR_ARG, "%s: chamber %d: mode %d is neither ADMM_PRESSURE_CONSTANT (0) nor ADMM_PRESSURE_GAS (1)", who, chamber, mode);
    if (!params) return fail(ctx, ADMM_ERR_ARG, "%s: chamber %d: params is NULL", who, chamber);
    static const char *const names[2][2] = {{"p", "params[1]"}, {"amount", "ambient"}};
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(params[k])) return fail(ctx, ADMM_ERR_ARG, "%s: chamber %d: %s %g is not finite", who, chamber, names[mode][k], params[k]);
    return ADMM_OK;
}

// gas mode: every edge is shared by exactly two triangles that run through it in opposite directions
static int pres_check_closed(admm_hip_ctx *ctx, const char *who, int chamber, const std::vector<int32_t> &tris) {
    std::vector<std::pair<int32_t, int32_t> > dir;      // the directed edges, sorted
    dir.reserve(tris.size());
    for (size_t t = 0; t < tris.size() / 3; ++t) for (int j = 0; j < 3; ++j) dir.push_back(std::make_pair(tris[3 * t + j], tris[3 * t + (j + 1) % 3]));
    std::sort(dir.begin(), dir.end());
    for (size_t i = 0; i < dir.size(); ++i) {
        const std::pair<int32_t, int32_t> e = dir[i], r = std::make_pair(e.second, e.first);
        const int same = (int)(std::upper_bound(dir.begin(), dir.end(), e) - std::lower_bound(dir.begin(), dir.end(), e));
        const int opposite = (int)(std::upper_bound(dir.begin(), dir.end(), r) - std::lower_bound(dir.begin(), dir.end(), r));
        if (same != 1 || opposite != 1)
            return fail(ctx, ADMM_ERR_ARG, "%s: chamber %d: a gas chamber must be closed, but edge (%d, %d) is run through %d times in that direction and %d times in the opposite one (1 and 1 wanted)",
                        who, chamber, (int)e.first, (int)e.second, same, opposite);
    }
    return ADMM_OK;
}

// admm_hip_finalize: a gas chamber's rest volume, from the node positions as they stand then, must be positive
static int check_pressure_chambers(admm_hip_ctx *ctx) {
    for (size_t c = 0; c < ctx->chambers.size(); ++c) {
        const admm_hip_ctx::PressureChamberHost &H = ctx->chambers[c];
        if (H.mode != ADMM_PRESSURE_GAS) continue;
        admm_pressure::Record R;
        admm_pressure::chamber_record(ctx->x.data(), H.tris.data(), (int64_t)(H.tris.size() / 3), H.mode, H.par[0], H.par[1], R, nullptr);
        if (!(R.volume > 0.0) || !std::isfinite(R.volume))
            return fail(ctx, ADMM_ERR_ARG, "finalize: chamber %d: a gas chamber needs a positive rest volume, but its triangles enclose %g (inward normals?)", (int)c, R.volume);
    }
    return ADMM_OK;
}

// the laws that changed since they last reached the device, as kernel arguments: no host buffer has to outlive the call
static void pres_flush_laws(admm_hip_ctx *ctx) {
    for (size_t c = 0; c < ctx->chambers.size(); ++c) {
        admm_hip_ctx::PressureChamberHost &H = ctx->chambers[c];
        if (!H.law_dirty) continue;
        hipLaunchKernelGGL(admm_dev::pressure_set_law_kernel, dim3(1), dim3(admm_dev::PRES_BLOCK), 0, ctx->stream, (admm_dev::PresLaw *)ctx->d_pres_law, (int)c, H.mode, H.par[0], H.par[1],
                           admm_pressure::active(H.mode, H.par[0], H.par[1]) ? 1 : 0);
        H.law_dirty = false;
    }
}

// admm_hip_step, after update_bodies / latch_sides and before the prologue: the load of every active chamber, three launches
static int launch_pressure(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    bool any = false;
    for (const admm_hip_ctx::PressureChamberHost &H : ctx->chambers) any = any || admm_pressure::active(H.mode, H.par[0], H.par[1]);
    if (!any) return ADMM_OK;
    pres_flush_laws(ctx);
    const PresDev d = pres_dev(ctx);
    hipLaunchKernelGGL(pressure_terms_kernel, dim3(ctx->pres_blocks), dim3(PRES_BLOCK), 0, ctx->stream, d, 0, 0, (const double *)ctx->d_x);
    hipLaunchKernelGGL(pressure_reduce_kernel, dim3((int)ctx->chambers.size()), dim3(PRES_REDUCE), 0, ctx->stream, d, 0, 0, 1);
    hipLaunchKernelGGL(pressure_apply_kernel, dim3((ctx->pres_nodes + PRES_APPLY - 1) / PRES_APPLY), dim3(PRES_APPLY), 0, ctx->stream, d, ctx->dt, (const double *)ctx->d_m3, ctx->d_v);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

int admm_hip_add_pressure_chamber(admm_hip_ctx *ctx, int nt, const int32_t *tris, int mode, const double *params, int *chamber) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "add_pressure_chamber: pressure chambers must be added before finalize");
    const int c = (int)ctx->chambers.size();
    if (nt < 1) return fail(ctx, ADMM_ERR_ARG, "add_pressure_chamber: chamber %d: nt %d is below 1", c, nt);
    if (!tris) return fail(ctx, ADMM_ERR_ARG, "add_pressure_chamber: chamber %d: tris is NULL", c);
    for (int t = 0; t < nt; ++t) {
        const int32_t *q = tris + 3 * (size_t)t;
        for (int j = 0; j < 3; ++j)
            if (q[j] < 0 || q[j] >= ctx->n_nodes) return fail(ctx, ADMM_ERR_ARG, "add_pressure_chamber: chamber %d: triangle %d names node %d, outside the %d nodes added so far", c, t, (int)q[j], ctx->n_nodes);
        if (q[0] == q[1] || q[1] == q[2] || q[0] == q[2]) return fail(ctx, ADMM_ERR_ARG, "add_pressure_chamber: chamber %d: triangle %d (%d, %d, %d) names a node twice", c, t, (int)q[0], (int)q[1], (int)q[2]);
    }
    TRY(pres_check_law(ctx, "add_pressure_chamber", c, mode, params));
    admm_hip_ctx::PressureChamberHost H;
    H.tris.assign(tris, tris + 3 * (size_t)nt);
    if (mode == ADMM_PRESSURE_GAS) TRY(pres_check_closed(ctx, "add_pressure_chamber", c, H.tris));
    H.mode = mode; H.par[0] = params[0]; H.par[1] = params[1]; H.law_dirty = true;
    ctx->chambers.push_back(H);
    if (chamber) *chamber = c;
    return ADMM_OK;
}

int admm_hip_set_pressure(admm_hip_ctx *ctx, int chamber, int mode, const double *params) {
    if (!ctx) return ADMM_ERR_ARG;
    if (chamber < 0 || chamber >= (int)ctx->chambers.size()) return fail(ctx, ADMM_ERR_ARG, "set_pressure: chamber %d is not a pressure chamber (have %d)", chamber, (int)ctx->chambers.size());
    TRY(pres_check_law(ctx, "set_pressure", chamber, mode, params));
    admm_hip_ctx::PressureChamberHost &H = ctx->chambers[chamber];
    if (mode == ADMM_PRESSURE_GAS && H.mode != ADMM_PRESSURE_GAS) TRY(pres_check_closed(ctx, "set_pressure", chamber, H.tris));
    H.mode = mode; H.par[0] = params[0]; H.par[1] = params[1]; H.law_dirty = true;      // (reaches the device with the next step's load)
    return ADMM_OK;
}

int admm_hip_get_chamber_state(admm_hip_ctx *ctx, int chamber, admm_hip_chamber_state *out) {
    if (!ctx || !out) return ADMM_ERR_ARG;
    if (chamber < 0 || chamber >= (int)ctx->chambers.size()) return fail(ctx, ADMM_ERR_ARG, "get_chamber_state: chamber %d is not a pressure chamber (have %d)", chamber, (int)ctx->chambers.size());
    if (ctx->device_id < 0) return fail(ctx, ADMM_ERR_STATE, "get_chamber_state: chamber %d: a host-only context (device_id %d) holds no state to sum; admm_hip_pressure_query evaluates the rule without a GPU", chamber, ctx->device_id);
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "get_chamber_state: chamber %d: admm_hip_finalize has not been called", chamber);
    static_assert(sizeof(admm_hip_chamber_state) == sizeof(admm_pressure::Record), "admm_hip_chamber_state is the device's record");
    HIPCHK(hipSetDevice(ctx->device_id));
    using namespace admm_dev;
    pres_flush_laws(ctx);
    int blk0 = 0;
    for (int k = 0; k < chamber; ++k) blk0 += ((int)(ctx->chambers[k].tris.size() / 3) + PRES_BLOCK - 1) / PRES_BLOCK;
    const int nblk = ((int)(ctx->chambers[chamber].tris.size() / 3) + PRES_BLOCK - 1) / PRES_BLOCK;
    const PresDev d = pres_dev(ctx);
    hipLaunchKernelGGL(pressure_terms_kernel, dim3(nblk), dim3(PRES_BLOCK), 0, ctx->stream, d, blk0, 1, (const double *)ctx->d_x);
    hipLaunchKernelGGL(pressure_reduce_kernel, dim3(1), dim3(PRES_REDUCE), 0, ctx->stream, d, chamber, 1, 0);
    HIPCHK(hipGetLastError());
    admm_hip_chamber_state R;
    HIPCHK(hipMemcpyAsync(&R, (const admm_pressure::Record *)ctx->d_pres_rec + chamber, sizeof R, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *out = R;
    return ADMM_OK;
}
