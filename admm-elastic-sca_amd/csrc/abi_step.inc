// abi_step.inc -- C ABI: weights, anchors, admm_hip_step (System::step, System.cpp:26-75), m_x / m_v access, the class API's frame boundary
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)

int admm_hip_set_weights(admm_hip_ctx *ctx, int batch, const double *weights) {
    if (!ctx || batch < 0 || batch >= (int)ctx->batches.size() || !weights) return ADMM_ERR_ARG;
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "set_weights before finalize");
    Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) std::copy(weights, weights + b.g_rows, b.g_roww.begin());
    else std::copy(weights, weights + b.n_total, b.weight.begin());
    return ADMM_OK;
}

static int recompute_weights(admm_hip_ctx *ctx) {
    TRY(host_assemble(ctx, true));
    TRY(host_factor(ctx, true));
    if (ctx->device_id >= 0) {
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        TRY(panels_to_device(ctx));
        if (ctx->dense && ctx->d_ainv) HIPCHK(hipMemcpy(ctx->d_ainv, ctx->Ainv.data(), ctx->Ainv.size() * sizeof(double), hipMemcpyHostToDevice));
        for (Batch &b : ctx->batches) {
            if (b.kind == ADMM_KIND_GENERIC) {
                std::vector<double> coef(b.g_sval.size());
                for (size_t i = 0; i < coef.size(); ++i) { const double w = b.g_roww[b.g_srow_b[i]]; coef[i] = b.g_sval[i] * ((ctx->dt * ctx->dt) * (w * w)); }
                if (!coef.empty()) HIPCHK(hipMemcpy(b.d_g_scoef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice));
                if (b.d_g_scoef_res && !coef.empty()) {
                    for (size_t i = 0; i < coef.size(); ++i) { const double w = b.g_roww[b.g_srow_b[i]]; coef[i] = b.g_sval[i] * (w * w); }
                    HIPCHK(hipMemcpy(b.d_g_scoef_res, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice));
                }
                continue;
            }
            const int nl = b.n_local;
            std::vector<double> w2h2(std::max(nl, 1)), w2(std::max(nl, 1));
            for (int el = 0; el < nl; ++el) { const double w = b.weight[b.local[el]]; w2[el] = w * w; w2h2[el] = (ctx->dt * ctx->dt) * (w * w); }
            if (nl) { HIPCHK(hipMemcpy(b.d_w2h2, w2h2.data(), sizeof(double) * nl, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(b.d_w2, w2.data(), sizeof(double) * nl, hipMemcpyHostToDevice)); }
        }
    }
    return ADMM_OK;
}

// a failure part-way leaves the panels (device: pivots replaced by 1.0), A^-1 or the weights of a half-done factorization: the factor stays
// marked invalid -- the steps refuse (require_factor) -- until a recompute_weights succeeds
int admm_hip_recompute_weights(admm_hip_ctx *ctx) {
    if (!ctx || !ctx->finalized) return ADMM_ERR_STATE;
    const int rc = recompute_weights(ctx);
    ctx->factor_invalid = rc != ADMM_OK;
    ctx->factor_error = rc ? ctx->err : std::string();
    return rc;
}

int admm_hip_update_anchors(admm_hip_ctx *ctx, int batch, const double *targets, const int32_t *active) {
    if (!ctx || batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    Batch &b = ctx->batches[batch];
    if (b.kind != ADMM_KIND_ANCHOR) return fail(ctx, ADMM_ERR_ARG, "batch %d is not an anchor batch", batch);
    if (targets && b.attach_body >= 0)      // (abi_attach.inc)
        return fail(ctx, ADMM_ERR_STATE, "update_anchors: batch %d is attached to rigid body %d, which rewrites its targets at every step: detach it first, or pass the flags alone", batch, b.attach_body);
    if (targets) std::copy(targets, targets + (size_t)3 * b.n_total, b.targets.begin());
    if (active) std::copy(active, active + b.n_total, b.active.begin());
    if (ctx->finalized && ctx->device_id >= 0 && b.n_local) {
        // asynchronous on the context's stream (it is ordered before the next step's kernels): this rank's targets / flags go
        // through a pinned staging buffer owned by the batch; the only wait is for the PREVIOUS update to have left that buffer
        HIPCHK(hipSetDevice(ctx->device_id));
        if (!b.h_tg) {
            HIPCHK(hipHostMalloc((void **)&b.h_tg, sizeof(double) * 3 * (size_t)b.n_local, hipHostMallocDefault));
            HIPCHK(hipHostMalloc((void **)&b.h_ac, sizeof(int32_t) * (size_t)b.n_local, hipHostMallocDefault));
            HIPCHK(hipEventCreateWithFlags(&b.upd_ev, hipEventDisableTiming));
        } else HIPCHK(hipEventSynchronize(b.upd_ev));
        for (int el = 0; el < b.n_local; ++el) { for (int j = 0; j < 3; ++j) b.h_tg[3 * (size_t)el + j] = b.targets[3 * (size_t)b.local[el] + j]; b.h_ac[el] = b.active[b.local[el]]; }
        if (targets) HIPCHK(hipMemcpyAsync(b.d_targets, b.h_tg, sizeof(double) * 3 * b.n_local, hipMemcpyHostToDevice, ctx->stream));
        if (active) HIPCHK(hipMemcpyAsync(b.d_active, b.h_ac, sizeof(int) * b.n_local, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipEventRecord(b.upd_ev, ctx->stream));
    }
    return ADMM_OK;
}

// records the next pooled event on the stream (timing mode only)
static int mark(admm_hip_ctx *ctx, bool on = true) {
    if (!ctx->timing || !on) return ADMM_OK;
    if (ctx->ev_used == ctx->evpool.size()) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ctx->evpool.push_back(e); }
    HIPCHK(hipEventRecord(ctx->evpool[ctx->ev_used++], ctx->stream));
    return ADMM_OK;
}

int admm_hip_step(admm_hip_ctx *ctx, int admm_iters) {
    TRY(require_factor(ctx));
    using namespace admm_dev;
    // Anderson acceleration (admm_hip_set_acceleration): refused before anything is launched, so that the state stands as it was
    const bool accel = ctx->aa_m > 0;
    if (accel && ctx->n_gen_rows) return fail(ctx, ADMM_ERR_UNSUPPORTED, "acceleration is not available in a context with user-defined (generic) batches: their z, u live on the host");
    if (accel && ctx->world > 1) return fail(ctx, ADMM_ERR_UNSUPPORTED, "acceleration is not available in a sharded context (world = %d): the Gram matrix would have to be all-reduced", ctx->world);
    HIPCHK(hipSetDevice(ctx->device_id));
    const int n3 = 3 * ctx->n_nodes;
    if (ctx->graphs_stale) { drop_iteration_graphs(ctx); ctx->graphs_stale = false; }      // the transport changed since the iteration was captured
    // event layout (timing mode): E0 | prologue (body surfaces' frame-start updates first) | E1 | per TIMED iteration: S local E rhs E allreduce E [exchange: E E] fwd E bwd E | Ea | epilogue | Eb
    if (ctx->timing) {      // the last step's events become "the previous step's" (still readable), the older set is recorded over
        ctx->evpool.swap(ctx->evpool_prev);
        ctx->ev_used_prev = ctx->ev_used; ctx->ev_iters_prev = ctx->ev_iters; ctx->ev_timed_prev = ctx->ev_timed; ctx->ev_pending_prev = ctx->ev_pending;
    } else ctx->ev_pending_prev = false;      // an untimed step: there is no timed "step before the last one" any more
    ctx->ev_used = 0; ctx->ev_iters = admm_iters; ctx->ev_timed = 0; ctx->ev_pending = ctx->timing;
    TRY(mark(ctx));
    if (!ctx->rigid.empty()) TRY(launch_rigid_pose(ctx));      // rigid bodies (abi_rigid.inc): their pose into the shape table, before anything reads it (eager, outside the graphs)
    if (ctx->d_body_tag) TRY(update_bodies(ctx));      // body surfaces from the frame-start x, before the explicit forces (eager, outside the graphs)
    if (ctx->d_side) TRY(latch_sides(ctx));            // side memory: every node's side from the frame-start x (eager, outside the graphs)
    if (!ctx->chambers.empty()) TRY(launch_pressure(ctx));      // pressure chambers (abi_pressure.inc): eager, from the frame-start x, into v before gravity and the wind
    if (ctx->frames++ > 0)      // the blocks of the large tet batches by what they cost in the frame before
        for (const Batch &b : ctx->batches) if (b.n_blocks_ordered)
            hipLaunchKernelGGL(order_by_cost_kernel, dim3(1), dim3(1024), 0, ctx->stream, b.n_blocks_ordered, b.d_cost, b.d_order);
    if (ctx->explicit_simple) {
        hipLaunchKernelGGL(prologue_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, n3, ctx->dt, ctx->grav, ctx->d_x, ctx->d_v, ctx->d_m3, ctx->d_mxbar, ctx->d_xcur);
    } else {
        for (const Explicit &E : ctx->explicits) {      // in list order, like System.cpp:37-39
            if (E.type == ADMM_EXPLICIT_CONST) {
                const int cnt = E.idx.empty() ? ctx->n_nodes : E.n;
                if (cnt) hipLaunchKernelGGL(explicit_const_kernel, dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, cnt, (const int *)E.d_idx, ctx->dt, E.dir[0], E.dir[1], E.dir[2], ctx->d_v);
            } else if (E.n) {
                hipLaunchKernelGGL(wind_serial_kernel, dim3(1), dim3(1024), 0, ctx->stream, E.n_levels, (const int *)E.d_level_ptr, (const int *)E.d_idx, ctx->dt, E.dir[0], E.dir[1], E.dir[2], ctx->d_x, ctx->d_v);
            }
        }
        hipLaunchKernelGGL(xbar_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, n3, ctx->dt, ctx->d_x, ctx->d_v, ctx->d_m3, ctx->d_mxbar, ctx->d_xcur);
    }
    TRY(mark(ctx));
    const bool track = ctx->res_on || ctx->tol_r > 0.0;
    if (track) TRY(ensure_residual_buffers(ctx, admm_iters));
    // Anderson acceleration (admm_hip_set_acceleration; abi_anderson.inc): the eager loop, the tets' z stored, its buffers before the loop
    if (accel) { TRY(ensure_anderson_buffers(ctx, admm_iters)); TRY(anderson_begin_frame(ctx)); }
    ctx->keep_z = ctx->keep_z_user || track || accel;
    // the per-iteration objective (admm_hip_enable_objective): its buffers exist before the loop, which then runs eagerly like a tracked one
    const bool objective = ctx->obj_on;
    if (objective && ctx->world > 1) return fail(ctx, ADMM_ERR_UNSUPPORTED, "the per-iteration objective is not available in a sharded context (world = %d)", ctx->world);
    if (objective) TRY(ensure_energy_buffers(ctx, admm_iters));
    ctx->obj_n = 0;
    if (!accel) ctx->aa_log_n = 0;      // (the log is the last step's)
    if (ctx->n_gen_rows) {      // user-defined forces: curr_z = D * m_x before the loop (System.cpp:43)
        TRY(generic_begin(ctx, ctx->d_x));
        HIPCHK(hipEventSynchronize(ctx->gen_ev));
        std::memcpy(ctx->h_gen_z, ctx->h_gen_dx, sizeof(double) * (size_t)ctx->n_gen_rows);
    }
    // world > 1: the iteration contains an all-reduce.  A host hook cannot be captured; ncclAllReduce can (RCCL collectives are
    // stream-ordered device work), so with the communicator inside the library the multi-GPU iteration is one graph launch too.
    const bool comm_capturable = ctx->world == 1 || (ctx->rccl_comm != nullptr && ctx->graph_comm);
    const bool use_graph = ctx->graph_enabled && (ctx->graph_forced || ctx->n_nodes < 100000) && comm_capturable && !(ctx->timing && ctx->timing_stride <= 1) && !track && !objective && !accel && admm_iters > 0 && !ctx->n_gen_rows;
    if (use_graph && !ctx->iter_exec) {   // capture one iteration; every kernel argument is a fixed device address
        // a stream that cannot be captured (caller-supplied, already capturing ...) is not an error: launch eagerly instead
        const hipError_t be = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
        int rc = be == hipSuccess ? launch_local(ctx) : ADMM_ERR_HIP;
        if (!rc) rc = launch_rhs(ctx);
        if (!rc && ctx->world > 1 && ctx->levels_top.empty()) rc = do_allreduce(ctx, ctx->d_y, (int64_t)n3);   // contiguous sharding (subtree: inside launch_solve)
        if (!rc) rc = launch_solve(ctx, nullptr);
        hipGraph_t g = nullptr;
        const hipError_t ce = be == hipSuccess ? hipStreamEndCapture(ctx->stream, &g) : be;
        if (rc || ce != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); ctx->graph_enabled = false; fprintf(stderr, "admm_hip: graph capture unavailable, launching eagerly\n"); }
        else {
            ctx->iter_graph = g;
            if (hipGraphInstantiate(&ctx->iter_exec, g, nullptr, nullptr, 0) != hipSuccess) { ctx->iter_exec = nullptr; (void)hipGraphDestroy(g); ctx->iter_graph = nullptr; (void)hipGetLastError(); ctx->graph_enabled = false; }
        }
    }
    // the frame's whole loop as one graph (no timing events inside; iteration counts beyond 64 keep the per-iteration graph)
    // (captured for an iteration count only once two calls in a row have asked for it: a caller that changes the count from frame to frame would
    //  otherwise pay a graph instantiation per frame)
    const bool same_count = admm_iters == ctx->last_step_iters;
    ctx->last_step_iters = admm_iters;
    const bool use_frame_graph = use_graph && ctx->iter_exec && ctx->frame_graph_on && !ctx->timing && admm_iters >= 2 && admm_iters <= 64 &&
                                 (same_count || (ctx->frame_exec && ctx->frame_iters == admm_iters));
    if (use_frame_graph && (!ctx->frame_exec || ctx->frame_iters != admm_iters)) {
        if (ctx->frame_exec) { (void)hipGraphExecDestroy(ctx->frame_exec); ctx->frame_exec = nullptr; }
        if (ctx->frame_graph) { (void)hipGraphDestroy(ctx->frame_graph); ctx->frame_graph = nullptr; }
        const hipError_t be = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
        int rc = be == hipSuccess ? ADMM_OK : ADMM_ERR_HIP;
        for (int it = 0; it < admm_iters && !rc; ++it) {
            rc = launch_local(ctx);
            if (!rc) rc = launch_rhs(ctx);
            if (!rc && ctx->world > 1 && ctx->levels_top.empty()) rc = do_allreduce(ctx, ctx->d_y, (int64_t)n3);
            if (!rc) rc = launch_solve(ctx, nullptr);
        }
        hipGraph_t g = nullptr;
        const hipError_t ce = be == hipSuccess ? hipStreamEndCapture(ctx->stream, &g) : be;
        if (rc || ce != hipSuccess || !g || hipGraphInstantiate(&ctx->frame_exec, g, nullptr, nullptr, 0) != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError(); ctx->frame_exec = nullptr; ctx->frame_graph_on = false;      // the per-iteration graph stays
        } else { ctx->frame_graph = g; ctx->frame_iters = admm_iters; }
    }
    ctx->res_n = 0;
    int iters_done = 0;
    const int stride = std::max(1, ctx->timing_stride);
    if (use_frame_graph && ctx->frame_exec && ctx->frame_iters == admm_iters) { HIPCHK(hipGraphLaunch(ctx->frame_exec, ctx->stream)); ++ctx->graph_launches; iters_done = admm_iters; }
    for (int it = iters_done; it < admm_iters; ++it) {
        // the sampled iterations rotate from frame to frame: an iteration's cost depends on its position in the frame (the first
        // ones after the prologue do the most line-search work), a fixed phase would bias the average
        const bool timed = ctx->timing && ((it + ctx->timing_frame) % stride == stride - 1);
        if (use_graph && ctx->iter_exec && !timed) { HIPCHK(hipGraphLaunch(ctx->iter_exec, ctx->stream)); ++ctx->graph_launches; iters_done = it + 1; continue; }
        if (timed) ++ctx->ev_timed;
        TRY(mark(ctx, timed));
        if (track) TRY(residual_snapshot(ctx, it == 0));
        if (accel) TRY(anderson_snapshot(ctx, it == 0));
        TRY(generic_begin(ctx, ctx->d_xcur));
        TRY(launch_local(ctx, -1, track));
        TRY(generic_finish(ctx));
        if (accel) {      // (inside the local-step interval of the timing events; the residuals first: they are measured on what the local step left)
            if (track) { TRY(launch_residuals(ctx, it)); ctx->res_n = it + 1; }
            TRY(anderson_accelerate(ctx, it, it + 1 == admm_iters));
            ctx->aa_log_n = it + 1;
        }
        TRY(mark(ctx, timed));
        if (track && !accel) { TRY(launch_residuals(ctx, it)); ctx->res_n = it + 1; }
        TRY(launch_rhs(ctx));
        TRY(mark(ctx, timed));
        if (ctx->world > 1 && ctx->levels_top.empty()) {     // contiguous sharding: the whole RHS is summed, the solve is replicated
            TRY(do_allreduce(ctx, ctx->d_y, (int64_t)n3));
        }
        TRY(mark(ctx, timed));
        // timing mode: one event between the sweeps; under subtree sharding two more around the exchange inside the forward
        // sweep (pack, all-reduce, unpack), so that allreduce_ms shows the communication and solve_fwd_ms only the sweeps
        // (distributed top: two more around the second exchange, the slices of the top's x)
        hipEvent_t mid = nullptr, ex0 = nullptr, ex1 = nullptr, ex2 = nullptr, ex3 = nullptr;
        if (timed) {
            const int want = ctx->levels_top.empty() ? 1 : (ctx->dist_top ? 5 : 3);
            while (ctx->ev_used + want > ctx->evpool.size()) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ctx->evpool.push_back(e); }
            if (want >= 3) { ex0 = ctx->evpool[ctx->ev_used++]; ex1 = ctx->evpool[ctx->ev_used++]; }
            if (want == 5) { ex2 = ctx->evpool[ctx->ev_used++]; ex3 = ctx->evpool[ctx->ev_used++]; }
            mid = ctx->evpool[ctx->ev_used++];
        }
        TRY(launch_solve(ctx, mid, ex0, ex1, ex2, ex3));
        TRY(mark(ctx, timed));
        if (objective) { TRY(launch_objective(ctx, it)); ctx->obj_n = it + 1; }      // inertia(x_k), elastic(x_k) of the x the global step just left
        iters_done = it + 1;
        if (ctx->tol_r > 0.0 && (it + 1) % ctx->check_every == 0 && it + 1 < admm_iters) {   // convergence test: one round trip
            double rs[2];
            HIPCHK(hipMemcpyAsync(rs, ctx->d_res + 2 * (size_t)it, sizeof rs, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (std::sqrt(rs[0]) <= ctx->tol_r && std::sqrt(rs[1]) <= ctx->tol_s) break;
        }
    }
    ctx->ev_iters = iters_done;
    if (ctx->timing) ++ctx->timing_frame;
    TRY(mark(ctx));
    TRY(shard_sync_x(ctx));
    hipLaunchKernelGGL(epilogue_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, n3, ctx->dt, ctx->d_x, ctx->d_v, ctx->d_xcur);
    HIPCHK(hipGetLastError());
    if (surface_reaction_any(ctx)) TRY(launch_surface_reaction(ctx));      // two-way contact (abi_surface_reaction.inc): eager, on the v the epilogue left, before the damping filter
    if (!ctx->rigid.empty()) TRY(launch_rigid_integrate(ctx));      // rigid bodies (abi_rigid.inc): eager, their contacts' reaction from the u, z, x the frame left, then one step of the rule
    if (!ctx->damp_groups.empty()) TRY(launch_damping(ctx));      // velocity damping per node group (abi_damping.inc): eager, on the v the epilogue left
    TRY(mark(ctx));
    if (ctx->rccl_comm) TRY(comm_poll(ctx, nullptr));      // once per frame: a dead peer becomes a failed step, not a hang in the caller's next sync
    return ADMM_OK;
}

int admm_hip_debug_graph_state(admm_hip_ctx *ctx, int *iter_graph, int *frame_graph, int64_t *graph_launches) {
    if (!ctx) return ADMM_ERR_ARG;
    if (iter_graph) *iter_graph = ctx->iter_exec != nullptr;
    if (frame_graph) *frame_graph = ctx->frame_exec ? ctx->frame_iters : 0;
    if (graph_launches) *graph_launches = ctx->graph_launches;
    return ADMM_OK;
}

// which kernels the collision batches launch for the current list (launch.inc: collision_form); 8 while contact attribution is on
int admm_hip_debug_collision_form(admm_hip_ctx *ctx, int *form) {
    if (!ctx || !form) return ADMM_ERR_ARG;
    *form = collision_form(ctx).form;
    return ADMM_OK;
}

// side memory (include/admm_hip.h): the sides of one mesh with memory, n_nodes values in the caller's node order (the device holds them in
// factor order; a host-only context keeps them on the host)
static int side_row(admm_hip_ctx *ctx, int mesh_id, int *row) {
    const admm_hip_ctx::CollisionMesh *m = mesh_by_id(ctx, mesh_id);
    if (!m) return ADMM_ERR_ARG;
    if (!(m->side_reach > 0.0)) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d has no side memory", mesh_id);
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "collision sides exist from finalize on");
    *row = m->side_row;
    return ADMM_OK;
}
int admm_hip_get_collision_sides(admm_hip_ctx *ctx, int mesh_id, int32_t *side) {
    if (!ctx || !side) return ADMM_ERR_ARG;
    int row = -1;
    TRY(side_row(ctx, mesh_id, &row));
    const size_t n = (size_t)ctx->n_nodes;
    if (ctx->device_id < 0) { std::copy(ctx->h_side.begin() + row * n, ctx->h_side.begin() + (row + 1) * n, side); return ADMM_OK; }
    HIPCHK(hipSetDevice(ctx->device_id));
    std::vector<int32_t> tmp(n);
    HIPCHK(hipMemcpyAsync(tmp.data(), ctx->d_side + row * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const std::vector<int> &perm = ctx->F.perm;
    for (size_t i = 0; i < n; ++i) side[perm[i]] = tmp[i];
    return ADMM_OK;
}
int admm_hip_set_collision_sides(admm_hip_ctx *ctx, int mesh_id, const int32_t *side) {
    if (!ctx || !side) return ADMM_ERR_ARG;
    int row = -1;
    TRY(side_row(ctx, mesh_id, &row));
    const size_t n = (size_t)ctx->n_nodes;
    for (size_t i = 0; i < n; ++i)
        if (side[i] < -1 || side[i] > 1) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: the side of node %d is %d: it must be -1, 0 or 1", mesh_id, (int)i, (int)side[i]);
    if (ctx->device_id < 0) { std::copy(side, side + n, ctx->h_side.begin() + row * n); return ADMM_OK; }
    HIPCHK(hipSetDevice(ctx->device_id));
    std::vector<int32_t> tmp(n);
    const std::vector<int> &perm = ctx->F.perm;
    for (size_t i = 0; i < n; ++i) tmp[i] = side[perm[i]];
    HIPCHK(hipMemcpyAsync(ctx->d_side + row * n, tmp.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}
// exactly the launches admm_hip_step begins with (body surfaces, then the latch) from the current x, synchronised
int admm_hip_latch_collision_sides(admm_hip_ctx *ctx) {
    TRY(require_device(ctx));
    HIPCHK(hipSetDevice(ctx->device_id));
    if (!ctx->rigid.empty()) TRY(launch_rigid_pose(ctx));
    if (ctx->d_body_tag) TRY(update_bodies(ctx));
    if (ctx->d_side) TRY(latch_sides(ctx));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}
int admm_hip_reset_collision_sides(admm_hip_ctx *ctx) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "collision sides exist from finalize on");
    std::fill(ctx->h_side.begin(), ctx->h_side.end(), 0);
    if (ctx->device_id >= 0 && ctx->d_side) {
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipMemsetAsync(ctx->d_side, 0, sizeof(int32_t) * (size_t)ctx->n_side_slots * (size_t)ctx->n_nodes, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return ADMM_OK;
}

int admm_hip_sync(admm_hip_ctx *ctx) {
    TRY(require_device(ctx));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}

static int get_nodes(admm_hip_ctx *ctx, const double *dsrc, double *out) {
    TRY(require_device(ctx));
    HIPCHK(hipSetDevice(ctx->device_id));
    std::vector<double> tmp(3 * (size_t)ctx->n_nodes);
    HIPCHK(hipMemcpyAsync(tmp.data(), dsrc, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const std::vector<int> &perm = ctx->F.perm;
    for (int i = 0; i < ctx->n_nodes; ++i) for (int c = 0; c < 3; ++c) out[3 * (size_t)perm[i] + c] = tmp[3 * (size_t)i + c];
    return ADMM_OK;
}
static int set_nodes(admm_hip_ctx *ctx, double *ddst, const double *in) {
    TRY(require_device(ctx));
    HIPCHK(hipSetDevice(ctx->device_id));
    std::vector<double> tmp(3 * (size_t)ctx->n_nodes);
    const std::vector<int> &perm = ctx->F.perm;
    for (int i = 0; i < ctx->n_nodes; ++i) for (int c = 0; c < 3; ++c) tmp[3 * (size_t)i + c] = in[3 * (size_t)perm[i] + c];
    HIPCHK(hipMemcpyAsync(ddst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}

int admm_hip_get_x(admm_hip_ctx *ctx, double *x) {
    if (ctx && !ctx->finalized && x) { std::copy(ctx->x.begin(), ctx->x.end(), x); return ADMM_OK; }
    if (ctx && ctx->finalized && ctx->device_id < 0 && x) { std::copy(ctx->x.begin(), ctx->x.end(), x); return ADMM_OK; }
    return x ? get_nodes(ctx, ctx ? ctx->d_x : nullptr, x) : ADMM_ERR_ARG;
}
int admm_hip_set_x(admm_hip_ctx *ctx, const double *x) {
    if (!ctx || !x) return ADMM_ERR_ARG;
    std::copy(x, x + ctx->x.size(), ctx->x.begin());
    if (!ctx->finalized || ctx->device_id < 0) return ADMM_OK;
    return set_nodes(ctx, ctx->d_x, x);
}
int admm_hip_get_v(admm_hip_ctx *ctx, double *v) {
    if (ctx && (!ctx->finalized || ctx->device_id < 0) && v) { std::copy(ctx->v.begin(), ctx->v.end(), v); return ADMM_OK; }
    return v ? get_nodes(ctx, ctx ? ctx->d_v : nullptr, v) : ADMM_ERR_ARG;
}
int admm_hip_set_v(admm_hip_ctx *ctx, const double *v) {
    if (!ctx || !v) return ADMM_ERR_ARG;
    std::copy(v, v + ctx->v.size(), ctx->v.begin());
    if (!ctx->finalized || ctx->device_id < 0) return ADMM_OK;
    return set_nodes(ctx, ctx->d_v, v);
}

// ---- frame boundary of the class API ------------------------------------------------------------------------
// One DMA per vector straight from / into the caller's memory (pinned with admm_hip_pin_host: full PCIe rate, truly
// asynchronous), the reordering between the caller's node order and the factor order on the device.
int admm_hip_pin_host(admm_hip_ctx *ctx, void *p, size_t bytes, int on) {
    if (!ctx || !p) return ADMM_ERR_ARG;
    if (ctx->device_id < 0) return ADMM_OK;
    HIPCHK(hipSetDevice(ctx->device_id));
    // a refused registration is not an error of the solver (pageable memory works, only slower): report it, clear HIP's
    // sticky last-error so that no later hipGetLastError() check trips over it, leave last_error alone
    const hipError_t e = on ? hipHostRegister(p, bytes, hipHostRegisterDefault) : hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return ADMM_ERR_HIP; }
    // the registered spans: the zero-copy state kernels address [x, x + 3 n doubles) -- a span that ends inside the vector must take the DMA path
    std::vector<std::pair<const char *, size_t> > &R = ctx->pinned;
    R.erase(std::remove_if(R.begin(), R.end(), [&](const std::pair<const char *, size_t> &q) { return q.first == (const char *)p; }), R.end());
    if (on) R.push_back({(const char *)p, bytes});
    return ADMM_OK;
}
// is [p, p + bytes) page-locked and device-addressable as ONE span?  A span registered through admm_hip_pin_host, or (memory the caller
// page-locked itself: hipHostMalloc / hipHostRegister) first AND last byte map to device addresses the same distance apart
static bool host_span_mapped(admm_hip_ctx *ctx, const void *p, size_t bytes, void **dev) {
    if (!p || !bytes) return false;
    if (hipHostGetDevicePointer(dev, (void *)p, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
    const char *c = (const char *)p;
    for (const std::pair<const char *, size_t> &q : ctx->pinned) if (c >= q.first && c + bytes <= q.first + q.second) return true;
    for (const std::pair<const char *, size_t> &q : ctx->pinned) if (c >= q.first && c < q.first + q.second) return false;      // starts inside a registered span that ends too early
    void *last = nullptr;
    if (hipHostGetDevicePointer(&last, (void *)(c + bytes - 1), 0) != hipSuccess) { (void)hipGetLastError(); return false; }
    return (const char *)last - (const char *)*dev == (ptrdiff_t)(bytes - 1);
}
// small systems: the page-locked [x | v] buffer the state kernels address directly (NULL: use the DMA path)
static double *state_buffer(admm_hip_ctx *ctx) {
    if (ctx->n_nodes > ctx->state_direct_max_nodes || !ctx->d_iperm) return nullptr;
    const size_t need = 6 * (size_t)ctx->n_nodes;
    if (ctx->h_state_cap < need) {
        if (ctx->h_state) { (void)hipStreamSynchronize(ctx->stream); (void)hipHostFree(ctx->h_state); ctx->h_state = nullptr; ctx->h_state_cap = 0; }
        void *dev = nullptr;
        if (hipHostMalloc((void **)&ctx->h_state, sizeof(double) * need, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dev, ctx->h_state, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (ctx->h_state) { (void)hipHostFree(ctx->h_state); ctx->h_state = nullptr; }
            ctx->state_direct_max_nodes = 0;      // no mapped host memory here: the DMA path from now on
            return nullptr;
        }
        ctx->h_state_dev = (double *)dev; ctx->h_state_cap = need;
        if (!ctx->state_in_ev && hipEventCreateWithFlags(&ctx->state_in_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ctx->state_direct_max_nodes = 0; return nullptr; }
    }
    return ctx->h_state;
}

// a vector that STARTS or ENDS inside a span registered through admm_hip_pin_host without lying inside it: HIP can neither map it nor copy it as
// one span (hipMemcpyAsync: invalid argument) -- it goes through a pageable copy owned by the context
static bool host_span_torn(const admm_hip_ctx *ctx, const void *p, size_t bytes) {
    const char *c = (const char *)p;
    for (const std::pair<const char *, size_t> &q : ctx->pinned) {
        const bool inside = c >= q.first && c + bytes <= q.first + q.second;
        const bool overlaps = c < q.first + q.second && c + bytes > q.first;
        if (overlaps && !inside) return true;
    }
    return false;
}

int admm_hip_upload_state(admm_hip_ctx *ctx, const double *x, const double *v) {
    TRY(require_device(ctx));
    HIPCHK(hipSetDevice(ctx->device_id));
    const int n3 = 3 * ctx->n_nodes;
    const size_t bytes = sizeof(double) * (size_t)n3;
    if (x && v) if (double *h = state_buffer(ctx)) {
        if (ctx->state_in_pending) { HIPCHK(hipEventSynchronize(ctx->state_in_ev)); ctx->state_in_pending = false; }      // the previous upload has left the buffer
        std::memcpy(h, x, bytes); std::memcpy(h + n3, v, bytes);
        hipLaunchKernelGGL(admm_dev::state_in_kernel, dim3((2 * n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_iperm, (const double *)ctx->h_state_dev, ctx->d_x, ctx->d_v);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->state_in_ev, ctx->stream)); ctx->state_in_pending = true;
        return ADMM_OK;
    }
    if (x && v && ctx->state_zero_copy && ctx->d_iperm) {      // the caller's page-locked vectors addressed by one kernel (no DMA, no staging)
        void *dx = nullptr, *dv = nullptr;
        if (host_span_mapped(ctx, x, bytes, &dx) && host_span_mapped(ctx, v, bytes, &dv)) {
            hipLaunchKernelGGL(admm_dev::state_in2_kernel, dim3(std::min((2 * n3 + 255) / 256, 4096)), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_iperm,
                               (const double *)dx, (const double *)dv, ctx->d_x, ctx->d_v);
            HIPCHK(hipGetLastError());
            return ADMM_OK;
        }
        // not page-locked as whole vectors (admm_hip_pin_host not called on them, or on fewer bytes): the DMA path below
    }
    const bool torn = (x && host_span_torn(ctx, x, bytes)) || (v && host_span_torn(ctx, v, bytes));
    if (torn) {      // (the copy must be complete before the call returns: the bounce buffer is reused)
        ctx->bounce.resize(2 * (size_t)n3);
        if (x) std::memcpy(ctx->bounce.data(), x, bytes);
        if (v) std::memcpy(ctx->bounce.data() + n3, v, bytes);
        x = x ? ctx->bounce.data() : nullptr; v = v ? ctx->bounce.data() + n3 : nullptr;
    }
    if (x) {
        HIPCHK(hipMemcpyAsync(ctx->d_stage, x, bytes, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(admm_dev::permute_in_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_perm, (const double *)ctx->d_stage, ctx->d_x);
    }
    if (v) {
        HIPCHK(hipMemcpyAsync(ctx->d_stage + n3, v, bytes, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(admm_dev::permute_in_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_perm, (const double *)(ctx->d_stage + n3), ctx->d_v);
    }
    HIPCHK(hipGetLastError());
    if (torn) HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}
int admm_hip_download_state(admm_hip_ctx *ctx, double *x, double *v) {
    TRY(require_device(ctx));
    HIPCHK(hipSetDevice(ctx->device_id));
    const int n3 = 3 * ctx->n_nodes;
    const size_t bytes = sizeof(double) * (size_t)n3;
    if (x && v) if (double *h = state_buffer(ctx)) {
        hipLaunchKernelGGL(admm_dev::state_out_kernel, dim3((2 * n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_iperm, (const double *)ctx->d_x, (const double *)ctx->d_v, ctx->h_state_dev);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));      // (also past any pending upload: the buffer is the host's again)
        ctx->state_in_pending = false;
        std::memcpy(x, h, bytes); std::memcpy(v, h + n3, bytes);
        return ADMM_OK;
    }
    if (x && v && ctx->state_zero_copy && ctx->d_iperm) {
        void *dx = nullptr, *dv = nullptr;
        if (host_span_mapped(ctx, x, bytes, &dx) && host_span_mapped(ctx, v, bytes, &dv)) {
            hipLaunchKernelGGL(admm_dev::state_out2_kernel, dim3(std::min((2 * n3 + 255) / 256, 4096)), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_iperm,
                               (const double *)ctx->d_x, (const double *)ctx->d_v, (double *)dx, (double *)dv);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(ctx->stream));
            return ADMM_OK;
        }
        (void)hipGetLastError();
    }
    const bool torn = (x && host_span_torn(ctx, x, bytes)) || (v && host_span_torn(ctx, v, bytes));
    double *ux = x, *uv = v;
    if (torn) { ctx->bounce.resize(2 * (size_t)n3); x = x ? ctx->bounce.data() : nullptr; v = v ? ctx->bounce.data() + n3 : nullptr; }
    if (x) {
        hipLaunchKernelGGL(admm_dev::permute_out_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_perm, (const double *)ctx->d_x, ctx->d_stage);
        HIPCHK(hipMemcpyAsync(x, ctx->d_stage, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (v) {
        hipLaunchKernelGGL(admm_dev::permute_out_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const int *)ctx->d_perm, (const double *)ctx->d_v, ctx->d_stage + n3);
        HIPCHK(hipMemcpyAsync(v, ctx->d_stage + n3, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (torn) { if (ux) std::memcpy(ux, x, bytes); if (uv) std::memcpy(uv, v, bytes); }
    return ADMM_OK;
}
