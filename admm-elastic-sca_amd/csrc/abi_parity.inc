// abi_parity.inc -- C ABI: parity / introspection entry points, residual and timing read-outs
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)

// SoA [rows][n] device -> element-major [n][rows] host
static int read_soa(admm_hip_ctx *ctx, const double *d, int rows, int n, double *out) {
    if (!out || n == 0) return ADMM_OK;
    std::vector<double> tmp((size_t)rows * n);
    HIPCHK(hipMemcpy(tmp.data(), d, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    to_element_major(tmp, rows, n, out);
    return ADMM_OK;
}

int admm_hip_read_local(admm_hip_ctx *ctx, int batch, double *u, double *z, double *state, int32_t *n_iters) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) {      // u, z of this rank's user forces, element after element (they live on the host)
        size_t o = 0;
        for (int el = 0; el < b.n_local; ++el) for (int64_t r = b.g_elem_row[b.local[el]]; r < b.g_elem_row[b.local[el] + 1]; ++r, ++o) {
            if (u) u[o] = ctx->h_gen_u[b.g_row0 + r];
            if (z) z[o] = ctx->h_gen_z[b.g_row0 + r];
        }
        return ADMM_OK;
    }
    const int rows = ADMM_KIND_ROWS[b.kind];
    TRY(read_soa(ctx, b.d_u, rows, b.n_local, u));
    TRY(read_soa(ctx, b.d_z, rows, b.n_local, z));
    if (state && ADMM_KIND_STATE[b.kind]) TRY(read_soa(ctx, b.d_state, 4, b.n_local, state));
    if (state && b.kind == ADMM_KIND_ANCHOR && b.n_local) HIPCHK(hipMemcpy(state, b.d_targets, sizeof(double) * 3 * b.n_local, hipMemcpyDeviceToHost));
    if (n_iters && b.n_local) HIPCHK(hipMemcpy(n_iters, b.d_niters, sizeof(int) * b.n_local, hipMemcpyDeviceToHost));
    return ADMM_OK;
}

int admm_hip_write_local(admm_hip_ctx *ctx, int batch, const double *u, const double *state) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) {
        size_t o = 0;
        if (u) for (int el = 0; el < b.n_local; ++el) for (int64_t r = b.g_elem_row[b.local[el]]; r < b.g_elem_row[b.local[el] + 1]; ++r, ++o) ctx->h_gen_u[b.g_row0 + r] = u[o];
        return ADMM_OK;
    }
    const int rows = ADMM_KIND_ROWS[b.kind], n = b.n_local;
    if (u && n) {
        std::vector<double> tmp((size_t)rows * n);
        for (int e = 0; e < n; ++e) for (int r = 0; r < rows; ++r) tmp[(size_t)r * n + e] = u[(size_t)e * rows + r];
        HIPCHK(hipMemcpy(b.d_u, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (state && n && ADMM_KIND_STATE[b.kind]) {
        std::vector<double> tmp((size_t)4 * n);
        for (int e = 0; e < n; ++e) for (int r = 0; r < 4; ++r) tmp[(size_t)r * n + e] = state[(size_t)e * 4 + r];
        HIPCHK(hipMemcpy(b.d_state, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return ADMM_OK;
}

int admm_hip_read_rest(admm_hip_ctx *ctx, int batch, double *weight, double *rest, int32_t *global_idx) {
    if (!ctx || !ctx->finalized || batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) { if (global_idx) std::copy(b.global_idx.begin(), b.global_idx.end(), global_idx); return ADMM_OK; }   // rest data and weights are the caller's
    if (weight) std::copy(b.weight.begin(), b.weight.end(), weight);
    if (rest) std::copy(b.rest.begin(), b.rest.end(), rest);
    if (global_idx) std::copy(b.global_idx.begin(), b.global_idx.end(), global_idx);
    return ADMM_OK;
}

int admm_hip_keep_z(admm_hip_ctx *ctx, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    if (getenv("ADMM_HIP_KEEP_Z")) return ADMM_OK;      // the environment decides
    if (ctx->keep_z_user != (on != 0)) {      // captured iterations carry the flag in their kernel arguments: capture again
        drop_iteration_graphs(ctx);
    }
    ctx->keep_z_user = on != 0;
    return ADMM_OK;
}

namespace { struct KeepZ { admm_hip_ctx *c; bool old; explicit KeepZ(admm_hip_ctx *c_) : c(c_), old(c_->keep_z) { c->keep_z = true; } ~KeepZ() { c->keep_z = old; } }; }

int admm_hip_local_step_only(admm_hip_ctx *ctx, const double *x_cur) {
    TRY(require_factor(ctx));
    if (!x_cur) return ADMM_ERR_ARG;
    KeepZ kz(ctx);
    TRY(set_nodes(ctx, ctx->d_xcur, x_cur));
    TRY(generic_begin(ctx, ctx->d_xcur));
    TRY(launch_local(ctx));
    TRY(generic_finish(ctx));
    TRY(launch_rhs(ctx));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}

// Parity-test hook: the right-hand side the last launch_rhs left in d_y, in the caller's node order -- after admm_hip_local_step_only
// exactly what the sweeps would be handed (this rank's vector, before any all-reduce).  NOT used by admm_hip_step or any product path.
int admm_hip_debug_rhs(admm_hip_ctx *ctx, double *y) {
    TRY(require_factor(ctx));
    if (!y) return ADMM_ERR_ARG;
    return get_nodes(ctx, ctx->d_y, y);
}

// Parity-test hook: one project() of every local element of `batch` on
// caller-supplied D_i x rows (element-major [n_local][rows]) instead of the
// gather from x -- replays the reference's recorded (Dx,u,state)->(u,z,state) tuples.
int admm_hip_local_step_dx(admm_hip_ctx *ctx, int batch, const double *dx) {
    TRY(require_factor(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size() || !dx) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) return fail(ctx, ADMM_ERR_UNSUPPORTED, "local_step_dx: a generic batch's project() is the caller's own code");
    if (b.n_local == 0) return ADMM_OK;
    SuppliedRows rows(ctx, b);
    TRY(rows.stage(dx));
    KeepZ kz(ctx);
    int rc = launch_local(ctx, batch);
    hipError_t e = rows.wait();
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, ADMM_ERR_HIP, "local_step_dx: %s", hipGetErrorString(e));
    return ADMM_OK;
}

int admm_hip_solve_only(admm_hip_ctx *ctx, const double *b, double *x) {
    TRY(require_factor(ctx));
    if (!b || !x) return ADMM_ERR_ARG;
    TRY(set_nodes(ctx, ctx->d_y, b));
    if (!ctx->levels_top.empty())   // subtree sharding sums the top rows over the ranks: every rank was handed the whole b, keep it once
        hipLaunchKernelGGL(admm_dev::shard_mask_nodes_kernel, dim3((3 * ctx->n_nodes + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const unsigned char *)ctx->d_keep_mask, ctx->d_y);
    TRY(launch_solve(ctx, nullptr));
    TRY(shard_sync_x(ctx));
    return get_nodes(ctx, ctx->d_xcur, x);
}

int admm_hip_apply_A(admm_hip_ctx *ctx, const double *x, double *y) {
    if (!ctx || !ctx->finalized || !x || !y) return ADMM_ERR_ARG;
    sym_apply(ctx->A, x, y);
    return ADMM_OK;
}

// Validation hook for the CPU test-suite: evaluates the two panel sweeps of
// factor.hpp on the host.  NOT used by admm_hip_step or any product path.
int admm_hip_debug_panel_solve_host(admm_hip_ctx *ctx, const double *b, double *x) {
    if (!ctx || !ctx->finalized || !b || !x) return ADMM_ERR_ARG;
    if (ctx->F.panels.empty() && ctx->factor_local_on) return fail(ctx, ADMM_ERR_STATE, "rank-local factorization: this rank holds only its own subtrees and the top, not the whole factor");
    if (ctx->F.panels.empty() && ctx->d_panels) {      // factored on the device: the host sweeps then check the DEVICE's factor
        ctx->F.panels.resize((size_t)ctx->F.panels_size);
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(ctx->F.panels.data(), ctx->d_panels, sizeof(double) * ctx->F.panels.size(), hipMemcpyDeviceToHost));
    }
    panel_solve_host(ctx->F, b, x);
    return ADMM_OK;
}

// Parity-test hook: ONE function of local_math.hpp per launch, as the device build of the header executes it, one lane per record.
// What the tests rely on (tests/test_device_math.py composes its waves from it): workgroups of 256 threads in one dimension, so record i
// runs on lane i % 64 of wave i / 64; a lane beyond n returns before any of the function's code (it is not in a __ballot inside it); op is
// a kernel argument, hence wave-uniform -- the switch below is a scalar branch and a launch runs one function.
// Records are element-major: in [n][ADMM_DEBUG_MATH_IN[op]], out [n][ADMM_DEBUG_MATH_OUT[op]]; matrices in column-major order
// (m00 m10 m20 m01 ...), the mt_cstep records as tests/host_math_shim.cpp hm_cstep_forms lays them out.
static const int ADMM_DEBUG_MATH_OPS = 10;
static const int ADMM_DEBUG_MATH_IN[ADMM_DEBUG_MATH_OPS] = {1, 1, 1, 1, 1, 2, 9, 9, 6, 12};
static const int ADMM_DEBUG_MATH_OUT[ADMM_DEBUG_MATH_OPS] = {1, 1, 1, 1, 1, 1, 21, 21, 12, 9};
namespace admm_dev {
__device__ __forceinline__ Mat3 debug_load3(const double *f) { Mat3 m; m.m00 = f[0]; m.m10 = f[1]; m.m20 = f[2]; m.m01 = f[3]; m.m11 = f[4]; m.m21 = f[5]; m.m02 = f[6]; m.m12 = f[7]; m.m22 = f[8]; return m; }
__device__ __forceinline__ void debug_store3(const Mat3 &m, double *f) { f[0] = m.m00; f[1] = m.m10; f[2] = m.m20; f[3] = m.m01; f[4] = m.m11; f[5] = m.m21; f[6] = m.m02; f[7] = m.m12; f[8] = m.m22; }
__global__ void __launch_bounds__(256) debug_math_kernel(int op, int64_t n, const double *__restrict__ in, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    switch (op) {
    case 0: out[i] = admm_log(in[i]); break;
    case 1: out[i] = admm_exp(in[i]); break;
    case 2: out[i] = sqrt_in_1_4(in[i]); break;
    case 3: out[i] = sqrt_ge_1(in[i]); break;
    case 4: out[i] = rcp_in_1_2(in[i]); break;
    case 5: out[i] = eig_hypot(in[2 * i], in[2 * i + 1]); break;
    case 6: case 7: {
        Mat3 U, V; double s0, s1, s2;
        if (op == 6) svd3(debug_load3(in + 9 * i), U, s0, s1, s2, V);
        else oriented_svd(debug_load3(in + 9 * i), s0, s1, s2, U, V);
        double *o = out + 21 * i;
        debug_store3(U, o); o[9] = s0; o[10] = s1; o[11] = s2; debug_store3(V, o + 12);
        break;
    }
    case 8: {
        double F[6], U2[6], V[4], s0, s1;
#pragma unroll
        for (int k = 0; k < 6; ++k) F[k] = in[6 * i + k];
        svd32(F, U2, s0, s1, V);
        double *o = out + 12 * i;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = U2[k];
        o[6] = s0; o[7] = s1;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[8 + k] = V[k];
        break;
    }
    default: {      // 9: in [stx fx dx sty fy dy stp fp dp stpmin stpmax brackt], out [stx fx dx sty fy dy stp brackt info]
        const double *a = in + 12 * i;
        double stx = a[0], fx = a[1], dx = a[2], sty = a[3], fy = a[4], dy = a[5], stp = a[6];
        bool brackt = a[11] != 0.0; int info = 0;
        mt_cstep(stx, fx, dx, sty, fy, dy, stp, a[7], a[8], brackt, a[9], a[10], info);
        double *o = out + 9 * i;
        o[0] = stx; o[1] = fx; o[2] = dx; o[3] = sty; o[4] = fy; o[5] = dy; o[6] = stp; o[7] = brackt; o[8] = info;
        break;
    }
    }
}
} // namespace admm_dev
int admm_hip_debug_gemm(admm_hip_ctx *ctx, int m, int n, int k, int lda, int ldb, int ldc, int flags, double alpha, double beta,
                        const double *A, int64_t size_a, const double *B, int64_t size_b, double *C, int64_t size_c) {
    TRY(require_device(ctx));
    if (!A || !B || !C || m < 1 || n < 1 || k < 1 || size_a < 1 || size_b < 1 || size_c < 1) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    double *dA = nullptr, *dB = nullptr, *dC = nullptr; admm_dev::GemmTask *dT = nullptr;
    auto done = [&](int rc) { for (void *p : {(void *)dA, (void *)dB, (void *)dC, (void *)dT}) if (p) (void)hipFree(p); return rc ? fail(ctx, rc, "debug_gemm failed") : ADMM_OK; };
    if (hipMalloc(&dA, 8 * size_a) != hipSuccess || hipMalloc(&dB, 8 * size_b) != hipSuccess || hipMalloc(&dC, 8 * size_c) != hipSuccess || hipMalloc(&dT, sizeof(admm_dev::GemmTask)) != hipSuccess) return done(ADMM_ERR_HIP);
    if (hipMemcpy(dA, A, 8 * size_a, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dB, B, 8 * size_b, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dC, C, 8 * size_c, hipMemcpyHostToDevice) != hipSuccess) return done(ADMM_ERR_HIP);
    admm_dev::GemmTask T{}; T.A = dA; T.B = dB; T.C = dC; T.m = m; T.n = n; T.k = k; T.lda = lda; T.ldb = ldb; T.ldc = ldc; T.flags = flags; T.alpha = alpha; T.beta = beta;
    if (hipMemcpy(dT, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return done(ADMM_ERR_HIP);
    hipLaunchKernelGGL(admm_dev::gemm_f64_kernel, dim3(((m + 63) / 64) * ((n + 63) / 64), 1), dim3(256), 0, ctx->stream, (const admm_dev::GemmTask *)dT);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(C, dC, 8 * size_c, hipMemcpyDeviceToHost) != hipSuccess) return done(ADMM_ERR_HIP);
    return done(ADMM_OK);
}
int admm_hip_debug_potrf_inv(admm_hip_ctx *ctx, int w, int ld, double *blk, double *out) {
    TRY(require_device(ctx));
    if (!blk || !out || w < 1 || w > 64 || ld < w) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    const size_t sz = 8 * (size_t)ld * w;
    double *dB = nullptr, *dO = nullptr; admm_dev::PotrfTask *dT = nullptr; int *dF = nullptr;
    auto done = [&](int rc) { for (void *p : {(void *)dB, (void *)dO, (void *)dT, (void *)dF}) if (p) (void)hipFree(p); return rc; };
    if (hipMalloc(&dB, sz) != hipSuccess || hipMalloc(&dO, sz) != hipSuccess || hipMalloc(&dT, sizeof(admm_dev::PotrfTask)) != hipSuccess || hipMalloc(&dF, sizeof(int)) != hipSuccess) return done(fail(ctx, ADMM_ERR_HIP, "debug_potrf_inv: hipMalloc"));
    admm_dev::PotrfTask T{}; T.blk = dB; T.out = dO; T.w = w; T.ld = ld; T.ldo = ld; T.id = 0;
    if (hipMemcpy(dB, blk, sz, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dO, 0, sz) != hipSuccess || hipMemset(dF, 0, sizeof(int)) != hipSuccess || hipMemcpy(dT, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return done(fail(ctx, ADMM_ERR_HIP, "debug_potrf_inv: copy"));
    hipLaunchKernelGGL(admm_dev::potrf_inv_kernel, dim3(1), dim3(256), 0, ctx->stream, (const admm_dev::PotrfTask *)dT, dF);
    int failed = 0;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(blk, dB, sz, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(out, dO, sz, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&failed, dF, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(ctx, ADMM_ERR_HIP, "debug_potrf_inv: run"));
    return done(failed ? fail(ctx, ADMM_ERR_FACTOR, "block is not positive definite") : ADMM_OK);
}
int admm_hip_debug_math(admm_hip_ctx *ctx, int op, int64_t n, const double *in, double *out) {
    TRY(require_device(ctx));
    if (!in || !out || n < 0 || n > (int64_t)1 << 30 || op < 0 || op >= ADMM_DEBUG_MATH_OPS) return ADMM_ERR_ARG;
    if (n == 0) return ADMM_OK;
    HIPCHK(hipSetDevice(ctx->device_id));
    const size_t sz_in = sizeof(double) * (size_t)n * ADMM_DEBUG_MATH_IN[op], sz_out = sizeof(double) * (size_t)n * ADMM_DEBUG_MATH_OUT[op];
    double *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc(&d_in, sz_in));
    if (hipMalloc(&d_out, sz_out) != hipSuccess) { (void)hipFree(d_in); return fail(ctx, ADMM_ERR_HIP, "hipMalloc failed"); }
    int rc = ADMM_OK;
    if (hipMemcpy(d_in, in, sz_in, hipMemcpyHostToDevice) != hipSuccess) rc = ADMM_ERR_HIP;
    if (!rc) {
        hipLaunchKernelGGL(admm_dev::debug_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, n, (const double *)d_in, d_out);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(out, d_out, sz_out, hipMemcpyDeviceToHost) != hipSuccess) rc = ADMM_ERR_HIP;
    }
    (void)hipFree(d_in); (void)hipFree(d_out);
    return rc ? fail(ctx, rc, "debug_math failed") : ADMM_OK;
}

int admm_hip_get_info(admm_hip_ctx *ctx, admm_hip_info *info) {
    if (!ctx || !info) return ADMM_ERR_ARG;
    *info = ctx->info;
    return ADMM_OK;
}

int admm_hip_enable_residuals(admm_hip_ctx *ctx, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    ctx->res_on = on != 0;
    return ADMM_OK;
}
int admm_hip_set_tolerance(admm_hip_ctx *ctx, double eps_r, double eps_s, int check_every) {
    if (!ctx || check_every < 1 || eps_r < 0.0 || eps_s < 0.0) return ADMM_ERR_ARG;
    ctx->tol_r = eps_r; ctx->tol_s = eps_s; ctx->check_every = check_every;
    return ADMM_OK;
}
int admm_hip_get_residuals(admm_hip_ctx *ctx, double *r_norm, double *s_norm, int capacity, int *n_iters) {
    TRY(require_device(ctx));
    if (capacity < 0 || (capacity && (!r_norm || !s_norm))) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int n = std::min(ctx->res_n, capacity);
    if (n > 0) {
        std::vector<double> h(2 * (size_t)n);
        HIPCHK(hipMemcpy(h.data(), ctx->d_res, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) { r_norm[i] = std::sqrt(h[2 * (size_t)i]); s_norm[i] = std::sqrt(h[2 * (size_t)i + 1]); }
    }
    if (n_iters) *n_iters = ctx->ev_iters;
    return ADMM_OK;
}
int admm_hip_enable_timing(admm_hip_ctx *ctx, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    ctx->timing = on != 0;
    ctx->timing_stride = on > 1 ? on : 1;      // on = k > 1: events around every k-th ADMM iteration only
    ctx->timing_frame = 0;
    // whatever an earlier timed stretch left behind is not "the last / the previous step" of the new setting: a read before the next
    // timed step reports ADMM_ERR_STATE instead of an old frame's events
    ctx->ev_pending = false; ctx->ev_pending_prev = false;
    return ADMM_OK;
}
// the events of one timed step -> phase times (waits for the step's last event)
static int read_timing(admm_hip_ctx *ctx, const std::vector<hipEvent_t> &E, size_t used, int timed, int iters, admm_hip_timing &T) {
    HIPCHK(hipSetDevice(ctx->device_id));
    const size_t per = ctx->levels_top.empty() ? 6 : (ctx->dist_top ? 10 : 8);       // events per TIMED ADMM iteration (see admm_hip_step)
    const size_t need = 4 + per * (size_t)timed;
    if (used != need) return fail(ctx, ADMM_ERR_STATE, "timing events incomplete (%zu of %zu)", used, need);
    HIPCHK(hipEventSynchronize(E[need - 1]));
    T = admm_hip_timing{};
    float v;
    HIPCHK(hipEventElapsedTime(&v, E[0], E[1])); T.prologue_ms = v;
    for (int it = 0; it < timed; ++it) {
        const size_t b = 2 + per * (size_t)it;
        HIPCHK(hipEventElapsedTime(&v, E[b], E[b + 1])); T.local_ms += v;
        HIPCHK(hipEventElapsedTime(&v, E[b + 1], E[b + 2])); T.rhs_ms += v;
        HIPCHK(hipEventElapsedTime(&v, E[b + 2], E[b + 3])); T.allreduce_ms += v;
        if (per == 10) {      // distributed top: E[b+3] solve start | E[b+4], E[b+5] first exchange | E[b+6], E[b+7] second exchange (the root's slice in between) | E[b+8] midpoint | E[b+9] solve end
            HIPCHK(hipEventElapsedTime(&v, E[b + 3], E[b + 4])); T.solve_fwd_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 4], E[b + 5])); T.allreduce_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 5], E[b + 6])); T.solve_fwd_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 6], E[b + 7])); T.allreduce_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 7], E[b + 8])); T.solve_fwd_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 8], E[b + 9])); T.solve_bwd_ms += v;
        } else if (per == 8) {      // E[b+3] solve start | E[b+4] exchange start | E[b+5] exchange end | E[b+6] sweeps' midpoint | E[b+7] solve end
            HIPCHK(hipEventElapsedTime(&v, E[b + 3], E[b + 4])); T.solve_fwd_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 4], E[b + 5])); T.allreduce_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 5], E[b + 6])); T.solve_fwd_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 6], E[b + 7])); T.solve_bwd_ms += v;
        } else {
            HIPCHK(hipEventElapsedTime(&v, E[b + 3], E[b + 4])); T.solve_fwd_ms += v;
            HIPCHK(hipEventElapsedTime(&v, E[b + 4], E[b + 5])); T.solve_bwd_ms += v;
        }
    }
    HIPCHK(hipEventElapsedTime(&v, E[need - 2], E[need - 1])); T.epilogue_ms = v;
    HIPCHK(hipEventElapsedTime(&v, E[0], E[need - 1])); T.total_ms = v;
    if (timed > 0 && timed != iters) {      // sampled: phase sums scaled to the whole frame (total_ms is the real span)
        const float sc = (float)iters / (float)timed;
        T.local_ms *= sc; T.rhs_ms *= sc; T.allreduce_ms *= sc; T.solve_fwd_ms *= sc; T.solve_bwd_ms *= sc;
    }
    T.iters = iters;
    return ADMM_OK;
}
// Reads back the events of the last step recorded in timing mode (waits for it).
int admm_hip_get_timing(admm_hip_ctx *ctx, admm_hip_timing *t) {
    if (!ctx || !t) return ADMM_ERR_ARG;
    if (ctx->ev_pending && ctx->device_id >= 0) {
        admm_hip_timing T{};
        TRY(read_timing(ctx, ctx->evpool, ctx->ev_used, ctx->ev_timed, ctx->ev_iters, T));
        ctx->last_timing = T;
        ctx->ev_pending = false;
    }
    *t = ctx->last_timing;
    return ADMM_OK;
}
// ... of the step BEFORE the last one: its events are long complete once another step has been queued behind it, so a loop
//   step(0); for f = 1 .. K-1 { step(f); get_timing_previous(); }  get_timing();
// reads every frame's phases without ever letting the GPU run dry between two frames (a host read-back at each frame's end costs the
// 1M-tet bar 0.2-0.3 ms of idle GPU per 13.5 ms frame).  ADMM_ERR_STATE if that step was not timed or has been read already.
int admm_hip_get_timing_previous(admm_hip_ctx *ctx, admm_hip_timing *t) {
    if (!ctx || !t) return ADMM_ERR_ARG;
    if (!ctx->ev_pending_prev || ctx->device_id < 0) return fail(ctx, ADMM_ERR_STATE, "no unread timing of the step before the last one");
    TRY(read_timing(ctx, ctx->evpool_prev, ctx->ev_used_prev, ctx->ev_timed_prev, ctx->ev_iters_prev, *t));
    ctx->ev_pending_prev = false;
    return ADMM_OK;
}
