// abi_damping.inc -- C ABI: velocity damping per node group (kernels_damping.hpp, damping.hpp) and the filter admm_hip_step launches
// after its epilogue
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  The filter writes v and nothing else of the solver's state; it runs eagerly on the context's
// stream, outside the captured iteration and frame graphs, and drops none of them.  A context with no group, or whose groups all have
// both rates zero, launches nothing here.

static admm_dev::DampDev damp_dev(const admm_hip_ctx *ctx) {
    admm_dev::DampDev d{};
    d.blocks = (const admm_dev::DampBlock *)ctx->d_damp_blk; d.groups = (const admm_dev::DampGroup *)ctx->d_damp_grp; d.rate = (const admm_dev::DampRate *)ctx->d_damp_rate;
    d.mom = (admm_damping::Moments *)ctx->d_damp_mom; d.vc = ctx->d_damp_vc; d.part = ctx->d_damp_part; d.n_blocks_total = ctx->damp_blocks;
    return d;
}

static int damp_check_rates(admm_hip_ctx *ctx, const char *who, int group, double drag, double internal) {
    if (!(drag >= 0.0) || !std::isfinite(drag)) return fail(ctx, ADMM_ERR_ARG, "%s: group %d: drag %g is negative or not finite", who, group, drag);
    if (!(internal >= 0.0) || !std::isfinite(internal)) return fail(ctx, ADMM_ERR_ARG, "%s: group %d: internal %g is negative or not finite", who, group, internal);
    return ADMM_OK;
}

// passes 1 and 2 with their reductions over the table's blocks [blk0, blk0 + nblk) and the groups [g0, g0 + ng) with mode >= which_min
static int launch_damping_moments(admm_hip_ctx *ctx, int blk0, int nblk, int g0, int ng, int which_min) {
    using namespace admm_dev;
    const DampDev d = damp_dev(ctx);
    hipLaunchKernelGGL(damping_pass_kernel<1>, dim3(nblk), dim3(DAMP_BLOCK), 0, ctx->stream, d, blk0, which_min, (const int *)ctx->d_iperm, (const double *)ctx->d_m3, (const double *)ctx->d_x, (const double *)ctx->d_v);
    hipLaunchKernelGGL(damping_reduce_kernel<1>, dim3(ng), dim3(DAMP_REDUCE), 0, ctx->stream, d, g0, which_min);
    hipLaunchKernelGGL(damping_pass_kernel<2>, dim3(nblk), dim3(DAMP_BLOCK), 0, ctx->stream, d, blk0, which_min, (const int *)ctx->d_iperm, (const double *)ctx->d_m3, (const double *)ctx->d_x, (const double *)ctx->d_v);
    hipLaunchKernelGGL(damping_reduce_kernel<2>, dim3(ng), dim3(DAMP_REDUCE), 0, ctx->stream, d, g0, which_min);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// admm_hip_step, directly after epilogue_kernel: the filter over every group with a rate above zero
static int launch_damping(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    bool any = false, any_internal = false;
    for (const admm_hip_ctx::DampGroupHost &H : ctx->damp_groups) { any = any || H.drag > 0.0 || H.internal > 0.0; any_internal = any_internal || H.internal > 0.0; }
    if (!any) return ADMM_OK;
    for (size_t g = 0; g < ctx->damp_groups.size(); ++g) {      // (the rates travel as kernel arguments: no host buffer has to outlive the call)
        admm_hip_ctx::DampGroupHost &H = ctx->damp_groups[g];
        if (!H.rate_dirty) continue;
        double beta, s;
        admm_damping::rates(H.drag, H.internal, ctx->dt, &beta, &s);
        hipLaunchKernelGGL(damping_set_rate_kernel, dim3(1), dim3(DAMP_BLOCK), 0, ctx->stream, (DampRate *)ctx->d_damp_rate, (int)g, beta, s, H.internal > 0.0 ? 2 : (H.drag > 0.0 ? 1 : 0));
        H.rate_dirty = false;
    }
    if (any_internal) TRY(launch_damping_moments(ctx, 0, ctx->damp_blocks, 0, (int)ctx->damp_groups.size(), 2));
    hipLaunchKernelGGL(damping_apply_kernel, dim3(ctx->damp_blocks), dim3(DAMP_BLOCK), 0, ctx->stream, damp_dev(ctx), (const int *)ctx->d_iperm, (const double *)ctx->d_x, ctx->d_v);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

int admm_hip_add_damping_group(admm_hip_ctx *ctx, int node_first, int node_count, double drag, double internal, int *group_id) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "add_damping_group: damping groups must be added before finalize");
    const int g = (int)ctx->damp_groups.size();
    if (node_count < 1) return fail(ctx, ADMM_ERR_ARG, "add_damping_group: group %d: node_count %d is below 1", g, node_count);
    if (node_first < 0 || (long long)node_first + node_count > (long long)ctx->n_nodes)
        return fail(ctx, ADMM_ERR_ARG, "add_damping_group: group %d: nodes [%d, %lld) lie outside the %d nodes added so far", g, node_first, (long long)node_first + node_count, ctx->n_nodes);
    for (int k = 0; k < g; ++k) {
        const admm_hip_ctx::DampGroupHost &O = ctx->damp_groups[k];
        if (node_first < O.node_first + O.node_count && O.node_first < node_first + node_count)
            return fail(ctx, ADMM_ERR_ARG, "add_damping_group: group %d, nodes [%d, %d), overlaps group %d, nodes [%d, %d)", g, node_first, node_first + node_count, k, O.node_first, O.node_first + O.node_count);
    }
    TRY(damp_check_rates(ctx, "add_damping_group", g, drag, internal));
    admm_hip_ctx::DampGroupHost H;
    H.node_first = node_first; H.node_count = node_count; H.drag = drag; H.internal = internal; H.rate_dirty = true;
    ctx->damp_groups.push_back(H);
    if (group_id) *group_id = g;
    return ADMM_OK;
}

int admm_hip_set_damping(admm_hip_ctx *ctx, int group, double drag, double internal) {
    if (!ctx) return ADMM_ERR_ARG;
    if (group < 0 || group >= (int)ctx->damp_groups.size()) return fail(ctx, ADMM_ERR_ARG, "set_damping: group %d is not a damping group (have %d)", group, (int)ctx->damp_groups.size());
    TRY(damp_check_rates(ctx, "set_damping", group, drag, internal));
    admm_hip_ctx::DampGroupHost &H = ctx->damp_groups[group];
    H.drag = drag; H.internal = internal; H.rate_dirty = true;      // (reaches the device with the next step's filter)
    return ADMM_OK;
}

int admm_hip_get_group_moments(admm_hip_ctx *ctx, int group, admm_hip_group_moments *out) {
    if (!ctx || !out) return ADMM_ERR_ARG;
    if (group < 0 || group >= (int)ctx->damp_groups.size()) return fail(ctx, ADMM_ERR_ARG, "get_group_moments: group %d is not a damping group (have %d)", group, (int)ctx->damp_groups.size());
    if (ctx->device_id < 0) return fail(ctx, ADMM_ERR_STATE, "get_group_moments: group %d: a host-only context (device_id %d) holds no state to sum; admm_hip_damping_query evaluates the rule without a GPU", group, ctx->device_id);
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "get_group_moments: group %d: admm_hip_finalize has not been called", group);
    static_assert(sizeof(admm_hip_group_moments) == sizeof(admm_damping::Moments), "admm_hip_group_moments is the device's record");
    HIPCHK(hipSetDevice(ctx->device_id));
    const admm_hip_ctx::DampGroupHost &H = ctx->damp_groups[group];
    int blk0 = 0;
    for (int k = 0; k < group; ++k) blk0 += (ctx->damp_groups[k].node_count + admm_dev::DAMP_BLOCK - 1) / admm_dev::DAMP_BLOCK;
    TRY(launch_damping_moments(ctx, blk0, (H.node_count + admm_dev::DAMP_BLOCK - 1) / admm_dev::DAMP_BLOCK, group, 1, 0));
    admm_hip_group_moments R;
    HIPCHK(hipMemcpyAsync(&R, (const admm_damping::Moments *)ctx->d_damp_mom + group, sizeof R, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *out = R;
    return ADMM_OK;
}
