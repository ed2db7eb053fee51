// abi_energy.inc -- C ABI: the elements' energies, the node terms and the per-iteration ADMM objective (kernels_energy.hpp, energy.hpp)
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  Nothing here writes x, v, u, z, the warm starts, the cost counters or the sides, and nothing
// drops a captured graph: the kernels read the state and write buffers of their own.

static bool energy_evaluated(const Batch &b) { return b.kind != ADMM_KIND_GENERIC && admm_energy::evaluated(b.kind); }
static int energy_blocks(int n) { return (n + admm_dev::ENERGY_BLOCK - 1) / admm_dev::ENERGY_BLOCK; }
// blocks of the constant explicit forces' partials, in list order
static int energy_gravity_blocks(const admm_hip_ctx *ctx) {
    int nb = 0;
    for (const Explicit &E : ctx->explicits) if (E.type == ADMM_EXPLICIT_CONST) nb += energy_blocks(E.idx.empty() ? ctx->n_nodes : E.n);
    return nb;
}

// every buffer the energy kernels write, created by the first call that needs one (admm_hip_step with the objective on: before its loop)
static int ensure_energy_buffers(admm_hip_ctx *ctx, int iters) {
    HIPCHK(hipSetDevice(ctx->device_id));
    const size_t nb = ctx->batches.size();
    if (!ctx->en_ready) {
        for (Batch &b : ctx->batches) {
            if (!energy_evaluated(b)) continue;
            const size_t nl = (size_t)std::max(b.n_local, 1), nblk = (size_t)std::max(energy_blocks(b.n_local), 1);
            TRY(dalloc(ctx, &b.d_eE, nl)); TRY(dalloc(ctx, &b.d_epart, nblk)); TRY(dalloc(ctx, &b.d_ecnt, nblk));
        }
        TRY(dalloc(ctx, &ctx->d_en_out, 3 + nb)); TRY(dalloc(ctx, &ctx->d_en_cnt, std::max<size_t>(nb, 1)));
        TRY(dalloc(ctx, &ctx->d_en_npart, (size_t)energy_blocks(ctx->n_nodes) + (size_t)energy_gravity_blocks(ctx) + 1));
        ctx->en_ready = true;
    }
    if (iters > ctx->obj_cap) { ctx->obj_cap = std::max(iters, 64); TRY(dalloc(ctx, &ctx->d_obj, (size_t)ctx->obj_cap * (1 + nb))); }
    return ADMM_OK;
}

// the per-element kernel of one batch's kind for the output o (EnergyOut: `what` = "energy", GradOut: "gradient") on the positions x
// (device order); an empty batch launches nothing.  (extern "C++": this file is included inside extern "C", where no template may stand)
extern "C++" {
template <class Out> static int launch_element_kernel(admm_hip_ctx *ctx, const Batch &b, const double *x, const Out &o, const char *what) {
    using namespace admm_dev;
    const int nblk = energy_blocks(b.n_local);
    if (!nblk) return ADMM_OK;
    ElementKernel<Out> k = nullptr;
    switch (b.kind) {
    case ADMM_KIND_TET_NH: k = tet_kernel<ADMM_KIND_TET_NH>(o); break;
    case ADMM_KIND_TET_STVK: k = tet_kernel<ADMM_KIND_TET_STVK>(o); break;
    case ADMM_KIND_TET_LINEAR: k = tet_kernel<ADMM_KIND_TET_LINEAR>(o); break;
    case ADMM_KIND_TET_VOLUME: k = tet_kernel<ADMM_KIND_TET_VOLUME>(o); break;
    case ADMM_KIND_TRI_STRAIN: k = tri_kernel<ADMM_KIND_TRI_STRAIN>(o); break;
    case ADMM_KIND_TRI_AREA: k = tri_kernel<ADMM_KIND_TRI_AREA>(o); break;
    case ADMM_KIND_TRI_FUNG: k = tri_kernel<ADMM_KIND_TRI_FUNG>(o); break;
    case ADMM_KIND_BEND: k = bend_kernel(o); break;
    case ADMM_KIND_SPRING: k = spring_kernel(o); break;
    case ADMM_KIND_ANCHOR: k = anchor_kernel(o); break;
    default: return fail(ctx, ADMM_ERR_UNSUPPORTED, "no %s is evaluated for kind %d", what, b.kind);
    }
    hipLaunchKernelGGL(k, dim3(nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, batch_dev(ctx, b), x, o);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}
} // extern "C++"

// the energy kernel of one batch on the positions x (device order), then -- total != null -- the batch's sum and count
static int launch_batch_energy(admm_hip_ctx *ctx, const Batch &b, const double *x, double *total, long long *count) {
    using namespace admm_dev;
    TRY(launch_element_kernel(ctx, b, x, EnergyOut{b.d_escale, b.d_eE, b.d_epart, b.d_ecnt}, "energy"));
    if (total) hipLaunchKernelGGL(energy_reduce_kernel, dim3(1), dim3(ENERGY_REDUCE), 0, ctx->stream, energy_blocks(b.n_local), (const double *)b.d_epart, (const int *)b.d_ecnt, total, count);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// a node term (0: kinetic from a = v, 1: inertia from a = x and the prologue's M x_bar) -> *out
static int launch_node_energy(admm_hip_ctx *ctx, int term, const double *a, double *out) {
    using namespace admm_dev;
    const int n = ctx->n_nodes, nblk = energy_blocks(n);
    if (nblk) {
        if (term == 0) hipLaunchKernelGGL(energy_node_kernel<0>, dim3(nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, n, (const int *)ctx->d_iperm, (const double *)ctx->d_m3, a, (const double *)nullptr, 0.5, ctx->d_en_npart);
        else hipLaunchKernelGGL(energy_node_kernel<1>, dim3(nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, n, (const int *)ctx->d_iperm, (const double *)ctx->d_m3, a, (const double *)ctx->d_mxbar, 1.0 / (2.0 * (ctx->dt * ctx->dt)), ctx->d_en_npart);
    }
    hipLaunchKernelGGL(energy_reduce_kernel, dim3(1), dim3(ENERGY_REDUCE), 0, ctx->stream, nblk, (const double *)ctx->d_en_npart, (const int *)nullptr, out, (long long *)nullptr);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}
// -sum m g x over every constant explicit force and its nodes (wind has no potential) -> *out
static int launch_gravity_energy(admm_hip_ctx *ctx, const double *x, double *out) {
    using namespace admm_dev;
    double *part = ctx->d_en_npart + energy_blocks(ctx->n_nodes);
    int at = 0;
    for (const Explicit &E : ctx->explicits) {
        if (E.type != ADMM_EXPLICIT_CONST) continue;
        const int cnt = E.idx.empty() ? ctx->n_nodes : E.n, nblk = energy_blocks(cnt);
        if (nblk) hipLaunchKernelGGL(energy_gravity_kernel, dim3(nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, cnt, (const int *)(E.idx.empty() ? nullptr : E.d_idx), (const int *)ctx->d_iperm,
                                     (const double *)ctx->d_m3, x, E.dir[0], E.dir[1], E.dir[2], part + at);
        at += nblk;
    }
    hipLaunchKernelGGL(energy_reduce_kernel, dim3(1), dim3(ENERGY_REDUCE), 0, ctx->stream, at, (const double *)part, (const int *)nullptr, out, (long long *)nullptr);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// admm_hip_step with the objective on, after the global step of iteration `it`: inertia(x_k) and every batch's total at x_k = d_xcur
static int launch_objective(admm_hip_ctx *ctx, int it) {
    double *row = ctx->d_obj + (size_t)it * (1 + ctx->batches.size());
    TRY(launch_node_energy(ctx, 1, ctx->d_xcur, row));
    for (size_t bi = 0; bi < ctx->batches.size(); ++bi) {
        const Batch &b = ctx->batches[bi];
        if (!energy_evaluated(b) || b.kind == ADMM_KIND_ANCHOR) continue;
        TRY(launch_batch_energy(ctx, b, ctx->d_xcur, row + 1 + bi, ctx->d_en_cnt + bi));
    }
    return ADMM_OK;
}

int admm_hip_energy(admm_hip_ctx *ctx, admm_hip_energy_totals *out) {
    TRY(require_device(ctx));
    if (!out) return ADMM_ERR_ARG;
    TRY(ensure_energy_buffers(ctx, 0));
    const size_t nb = ctx->batches.size();
    int64_t skipped = 0;
    for (size_t bi = 0; bi < nb; ++bi) {
        const Batch &b = ctx->batches[bi];
        if (!energy_evaluated(b)) { ++skipped; continue; }
        TRY(launch_batch_energy(ctx, b, ctx->d_x, ctx->d_en_out + 3 + bi, ctx->d_en_cnt + bi));
    }
    TRY(launch_node_energy(ctx, 0, ctx->d_v, ctx->d_en_out));
    TRY(launch_gravity_energy(ctx, ctx->d_x, ctx->d_en_out + 1));
    std::vector<double> h(3 + nb, 0.0); std::vector<long long> c(std::max<size_t>(nb, 1), 0);
    HIPCHK(hipMemcpyAsync(h.data(), ctx->d_en_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(c.data(), ctx->d_en_cnt, sizeof(long long) * c.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    admm_hip_energy_totals T{};
    T.kinetic = h[0]; T.gravity = h[1]; T.batches_skipped = skipped;
    for (size_t bi = 0; bi < nb; ++bi) {      // in batch order
        const Batch &b = ctx->batches[bi];
        if (!energy_evaluated(b)) continue;
        if (b.kind == ADMM_KIND_ANCHOR) T.anchor += h[3 + bi]; else T.elastic += h[3 + bi];
        T.n_infinite += c[bi];
    }
    *out = T;
    return ADMM_OK;
}

int admm_hip_batch_energy(admm_hip_ctx *ctx, int batch, double *total, double *per_elem, int64_t *n_infinite) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (!energy_evaluated(b)) {      // collision and user-defined batches: not evaluated, the value is 0
        if (total) *total = 0.0;
        if (n_infinite) *n_infinite = 0;
        if (per_elem && b.kind != ADMM_KIND_GENERIC) std::fill(per_elem, per_elem + b.n_local, 0.0);
        return ADMM_OK;
    }
    TRY(ensure_energy_buffers(ctx, 0));
    TRY(launch_batch_energy(ctx, b, ctx->d_x, ctx->d_en_out + 3 + batch, ctx->d_en_cnt + batch));
    double t = 0.0; long long c = 0;
    HIPCHK(hipMemcpyAsync(&t, ctx->d_en_out + 3 + batch, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&c, ctx->d_en_cnt + batch, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (per_elem && b.n_local) HIPCHK(hipMemcpyAsync(per_elem, b.d_eE, sizeof(double) * (size_t)b.n_local, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (total) *total = t;
    if (n_infinite) *n_infinite = c;
    return ADMM_OK;
}

// parity entry: the same kernel on caller-supplied D_i x rows (element-major [n_local][rows]) instead of the gather, like admm_hip_local_step_dx
int admm_hip_batch_energy_dx(admm_hip_ctx *ctx, int batch, const double *dx, double *per_elem) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size() || !dx) return ADMM_ERR_ARG;
    Batch &b = ctx->batches[batch];
    if (!energy_evaluated(b)) return fail(ctx, ADMM_ERR_UNSUPPORTED, "batch_energy_dx: no energy is evaluated for batch %d (kind %d)", batch, b.kind);
    TRY(ensure_energy_buffers(ctx, 0));
    if (b.n_local == 0) return ADMM_OK;
    SuppliedRows rows(ctx, b);
    TRY(rows.stage(dx));
    TRY(launch_batch_energy(ctx, b, ctx->d_x, nullptr, nullptr));
    if (per_elem) HIPCHK(hipMemcpyAsync(per_elem, b.d_eE, sizeof(double) * (size_t)b.n_local, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(rows.wait());
    return ADMM_OK;
}

// this rank's elements' scale s, in the order of admm_hip_read_local
int admm_hip_read_energy_scale(admm_hip_ctx *ctx, int batch, double *s) {
    if (!ctx || !ctx->finalized || batch < 0 || batch >= (int)ctx->batches.size() || !s) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC) return fail(ctx, ADMM_ERR_UNSUPPORTED, "read_energy_scale: a generic batch has no energy");
    for (int el = 0; el < b.n_local; ++el) s[el] = energy_scale(b, b.local[el]);
    return ADMM_OK;
}

int admm_hip_enable_objective(admm_hip_ctx *ctx, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    if (on && ctx->world > 1) return fail(ctx, ADMM_ERR_UNSUPPORTED, "the per-iteration objective is not available in a sharded context (world = %d): under subtree shards the full x exists only at the end of the frame", ctx->world);
    ctx->obj_on = on != 0;
    return ADMM_OK;
}

int admm_hip_get_objective(admm_hip_ctx *ctx, double *inertia, double *elastic, int capacity, int *n_iters) {
    TRY(require_device(ctx));
    if (capacity < 0 || (capacity && (!inertia || !elastic))) return ADMM_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int n = std::min(ctx->obj_n, capacity);
    const size_t nb = ctx->batches.size(), w = 1 + nb;
    if (n > 0) {
        std::vector<double> h((size_t)n * w);
        HIPCHK(hipMemcpy(h.data(), ctx->d_obj, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            inertia[i] = h[(size_t)i * w];
            double e = 0.0;      // the batch totals in batch order, as admm_hip_energy adds them
            for (size_t bi = 0; bi < nb; ++bi) if (energy_evaluated(ctx->batches[bi]) && ctx->batches[bi].kind != ADMM_KIND_ANCHOR) e += h[(size_t)i * w + 1 + bi];
            elastic[i] = e;
        }
    }
    if (n_iters) *n_iters = ctx->obj_n;
    return ADMM_OK;
}
