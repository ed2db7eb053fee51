// abi_anderson.inc -- C ABI and launches: Anderson acceleration of the ADMM iteration (kernels_anderson.hpp, anderson.hpp)
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  With the window at 0 (the default) nothing here runs and nothing is allocated.

static int read_soa(admm_hip_ctx *ctx, const double *d, int rows, int n, double *out);      // (abi_parity.inc)

static void anderson_free(admm_hip_ctx *ctx, void *p) {
    if (!p) return;
    (void)hipFree(p);
    ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), p), ctx->allocs.end());
}

// the segment table, s_in, the partials and the decision state once; the two rings for the window (again when it grows); the log for
// `iters` records
static int ensure_anderson_buffers(admm_hip_ctx *ctx, int iters) {
    using namespace admm_dev;
    HIPCHK(hipSetDevice(ctx->device_id));
    if (!ctx->d_aa_seg) {
        std::vector<AASeg> segs;
        long long off = 0; int blk = 0;
        for (Batch &b : ctx->batches) {
            if (b.kind == ADMM_KIND_GENERIC || !b.n_local) continue;
            const long long cnt = (long long)ADMM_KIND_ROWS[b.kind] * b.n_local;
            if (cnt >= (1ll << 31) - AA_PER_BLOCK) return fail(ctx, ADMM_ERR_UNSUPPORTED, "acceleration: a batch of %lld rows is beyond the kernels' 32-bit element index", cnt);
            if (!b.d_G) TRY(upload(ctx, &b.d_G, b.G));      // (residual tracking uploads it too: whoever comes first)
            for (int part = 0; part < 2; ++part) {
                AASeg s{};
                s.live = part ? b.d_u : b.d_z; s.w2 = b.d_w2; s.n_local = (unsigned int)b.n_local; s.cnt = (unsigned int)cnt;
                s.blk0 = blk; blk += (int)((cnt + AA_PER_BLOCK - 1) / AA_PER_BLOCK); s.blk1 = blk; s.off = off;
                (part ? b.aa_off_u : b.aa_off_z) = off;
                off += cnt + (cnt & 1);
                segs.push_back(s);
            }
        }
        ctx->aa_nblk = blk; ctx->aa_T = off;
        AASeg *d = nullptr;
        TRY(upload(ctx, &d, segs));
        ctx->d_aa_seg = d;
        AAState *st = nullptr;
        TRY(dalloc(ctx, &st, 1));
        ctx->d_aa_state = st;
        TRY(dalloc(ctx, &ctx->d_aa_sin, (size_t)std::max<long long>(off, 1)));
        TRY(dalloc(ctx, &ctx->d_aa_part, (size_t)AA_NSUM * std::max(blk, 1)));
    }
    if (ctx->aa_m > ctx->aa_cap_m) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        anderson_free(ctx, ctx->d_aa_ring); ctx->d_aa_ring = nullptr; ctx->aa_cap_m = 0; ctx->aa_ran = false;
        TRY(dalloc(ctx, &ctx->d_aa_ring, 2 * (size_t)(ctx->aa_m + 1) * (size_t)std::max<long long>(ctx->aa_T, 1)));
        ctx->aa_cap_m = ctx->aa_m;
    }
    if (iters > ctx->aa_log_cap) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        anderson_free(ctx, ctx->d_aa_log); ctx->d_aa_log = nullptr;
        ctx->aa_log_cap = std::max(iters, 64);
        TRY(dalloc(ctx, &ctx->d_aa_log, (size_t)ctx->aa_log_cap));
    }
    return ADMM_OK;
}

// the two rings of the current window inside d_aa_ring
static double *anderson_ring_g(const admm_hip_ctx *ctx) { return ctx->d_aa_ring; }
static double *anderson_ring_f(const admm_hip_ctx *ctx) { return ctx->d_aa_ring + (size_t)(ctx->aa_m + 1) * (size_t)ctx->aa_T; }

// a frame starts with an empty history and an unconditional accept
static int anderson_begin_frame(admm_hip_ctx *ctx) {
    HIPCHK(hipMemsetAsync(ctx->d_aa_state, 0, sizeof(admm_dev::AAState), ctx->stream));
    ctx->aa_log_n = 0; ctx->aa_ran = true;
    return ADMM_OK;
}

// before the local step: s_in <- (z, u); at a frame's first iteration z = D x (System.cpp:43), as residual tracking takes it
static int anderson_snapshot(admm_hip_ctx *ctx, bool first_iteration) {
    using namespace admm_dev;
    if (!ctx->aa_nblk) return ADMM_OK;
    hipLaunchKernelGGL(anderson_snapshot_kernel, dim3(ctx->aa_nblk), dim3(AA_BLOCK), 0, ctx->stream, (const AASeg *)ctx->d_aa_seg, ctx->d_aa_sin);
    if (first_iteration)
        for (const Batch &b : ctx->batches) {
            if (b.kind == ADMM_KIND_GENERIC || !b.n_local) continue;
            hipLaunchKernelGGL(residual_dx_kernel, dim3((b.n_local + RES_BLOCK - 1) / RES_BLOCK), dim3(RES_BLOCK), 0, ctx->stream,
                               b.n_local, ADMM_KIND_NODES[b.kind], ADMM_KIND_ROWS[b.kind] / 3, idx_stride(b.kind), b.d_idx, b.d_G, ctx->d_x, ctx->d_aa_sin + b.aa_off_z);
        }
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// after the local step of iteration `it`, before the right-hand side: residual and dots, the decision, s_out -> z, u, the shares again
static int anderson_accelerate(admm_hip_ctx *ctx, int it, bool last) {
    using namespace admm_dev;
    if (!ctx->aa_nblk) return ADMM_OK;
    const hipStream_t st = ctx->stream;
    const AASeg *segs = (const AASeg *)ctx->d_aa_seg;
    AAState *state = (AAState *)ctx->d_aa_state;
    const int m = ctx->aa_m;
    hipLaunchKernelGGL(anderson_residual_kernel, dim3(ctx->aa_nblk), dim3(AA_BLOCK), 0, st, segs, (const AAState *)state, m, ctx->aa_T, (const double *)ctx->d_aa_sin,
                       anderson_ring_g(ctx), anderson_ring_f(ctx), ctx->aa_nblk, ctx->d_aa_part);
    hipLaunchKernelGGL(anderson_decide_kernel, dim3(1), dim3(AA_BLOCK), 0, st, state, m, ctx->aa_nblk, (const double *)ctx->d_aa_part, last ? 1 : 0, ctx->d_aa_log + it);
    hipLaunchKernelGGL(anderson_mix_kernel, dim3(ctx->aa_nblk), dim3(AA_BLOCK), 0, st, segs, (const AAState *)state, ctx->aa_T, (const double *)anderson_ring_g(ctx));
    for (const Batch &b : ctx->batches) {
        if (b.kind == ADMM_KIND_GENERIC || !b.n_local) continue;
        if (b.prered) {
            const BatchDev d = batch_dev(ctx, b);
            hipLaunchKernelGGL(anderson_reslot_tet_kernel, dim3(batch_blocks(b)), dim3(LOCAL_BLOCK), 0, st, (const AAState *)state, d, (const double *)b.d_G);
        } else
            hipLaunchKernelGGL(anderson_reslot_kernel, dim3((b.n_local + RES_BLOCK - 1) / RES_BLOCK), dim3(RES_BLOCK), 0, st, (const AAState *)state, b.n_local, ADMM_KIND_NODES[b.kind],
                               ADMM_KIND_ROWS[b.kind] / 3, idx_stride(b.kind), (const double *)b.d_z, (const double *)b.d_u, (const double *)b.d_w2h2, (const double *)b.d_G,
                               (const int *)b.d_dst, ctx->d_fslot);
    }
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

int admm_hip_set_acceleration(admm_hip_ctx *ctx, int window) {
    if (!ctx) return ADMM_ERR_ARG;
    if (window < 0 || window > admm_dev::AA_MAX_M) return fail(ctx, ADMM_ERR_ARG, "set_acceleration: the window must be 0 .. %d, got %d", admm_dev::AA_MAX_M, window);
    ctx->aa_m = window;
    return ADMM_OK;
}

int admm_hip_get_acceleration_log(admm_hip_ctx *ctx, admm_hip_acceleration_record *records, int capacity, int *n) {
    TRY(require_device(ctx));
    if (capacity < 0 || (capacity && !records)) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int k = std::min(ctx->aa_log_n, capacity);
    if (k > 0) HIPCHK(hipMemcpy(records, ctx->d_aa_log, sizeof(admm_hip_acceleration_record) * (size_t)k, hipMemcpyDeviceToHost));
    if (n) *n = ctx->aa_log_n;
    return ADMM_OK;
}

int admm_hip_get_acceleration_default(admm_hip_ctx *ctx, int batch, double *z, double *u) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) return fail(ctx, ADMM_ERR_UNSUPPORTED, "acceleration_default: a generic batch is not part of the accelerated state");
    if (!ctx->aa_ran || !ctx->d_aa_ring) return fail(ctx, ADMM_ERR_STATE, "acceleration_default: no accelerated step has run (admm_hip_set_acceleration, then admm_hip_step)");
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    admm_dev::AAState st;
    HIPCHK(hipMemcpy(&st, ctx->d_aa_state, sizeof st, hipMemcpyDeviceToHost));
    // (the ring of the window the last accelerated step ran with: aa_cap_m slots or fewer -- its slot stride is that step's window)
    const double *g = ctx->d_aa_ring + (size_t)st.def_slot * (size_t)ctx->aa_T;
    const int rows = ADMM_KIND_ROWS[b.kind];
    TRY(read_soa(ctx, g + b.aa_off_z, rows, b.n_local, z));
    TRY(read_soa(ctx, g + b.aa_off_u, rows, b.n_local, u));
    return ADMM_OK;
}
