// abi_gradient.inc -- C ABI: the elements' gradients g = dE/dd, their corner forces, the tets' stress and the nodes' internal forces
// (kernels_gradient.hpp, gradient.hpp)
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  Nothing here writes x, v, u, z, the warm starts, the cost counters or the sides, and nothing
// drops a captured graph: the kernels read the state and write buffers of their own.  Every copy and fill is asynchronous on the
// context's stream, which the call then waits for (DESIGN.md section 7, "Streams").

// every buffer the element kernels write, created by the first call that needs one
static int ensure_gradient_buffers(admm_hip_ctx *ctx) {
    HIPCHK(hipSetDevice(ctx->device_id));
    if (ctx->gr_ready) return ADMM_OK;
    long long total = 0;      // (what a call that failed further down allocated is reused)
    for (Batch &b : ctx->batches) {
        if (!energy_evaluated(b)) continue;
        const size_t nl = (size_t)std::max(b.n_local, 1);
        if (!b.d_gg) TRY(dalloc(ctx, &b.d_gg, (size_t)ADMM_KIND_ROWS[b.kind] * nl));
        if (!b.d_gcnt) TRY(dalloc(ctx, &b.d_gcnt, (size_t)std::max(energy_blocks(b.n_local), 1)));
        b.gr_cf_off = total;
        total += 3ll * ADMM_KIND_NODES[b.kind] * (long long)nl;
    }
    if (!ctx->d_gr_cf) TRY(dalloc(ctx, &ctx->d_gr_cf, (size_t)std::max(total, 1ll)));
    if (!ctx->d_gr_out) TRY(dalloc(ctx, &ctx->d_gr_out, 6 * (size_t)std::max(ctx->n_nodes, 1)));
    ctx->gr_ready = true;
    return ADMM_OK;
}

// a tet batch's stress buffer and its rest volumes (Batch::measure), at the first admm_hip_batch_stress of the batch
static int ensure_stress_buffers(admm_hip_ctx *ctx, Batch &b) {
    if (b.d_gstress) return ADMM_OK;
    const size_t nl = (size_t)std::max(b.n_local, 1);
    std::vector<double> vol(nl, 0.0);
    for (int el = 0; el < b.n_local; ++el) vol[el] = b.measure[b.local[el]];
    if (!b.d_gvol) TRY(dalloc(ctx, &b.d_gvol, nl));      // (a call that failed further down left it: reused)
    HIPCHK(hipMemcpyAsync(b.d_gvol, vol.data(), sizeof(double) * nl, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // (vol leaves scope)
    TRY(dalloc(ctx, &b.d_gstress, 7 * nl));      // last: its presence says that both are ready
    return ADMM_OK;
}

// stored corner (the device's order) of the element's original corner c
static int stored_corner(const Batch &b, int e, int c) {
    const int nn = ADMM_KIND_NODES[b.kind];
    for (int sc = 0; sc < nn; ++sc) if (b.corner_perm[(size_t)e * nn + sc] == c) return sc;
    return c;
}

// a gather kernel's CSR (node_csr.hpp) to the device, on the context's stream: the three arrays are created at first use (a call that
// failed further down left what it had allocated: reused, the sizes depend on the scene alone), and the call waits, since h is the caller's
static int upload_node_csr(admm_hip_ctx *ctx, const NodeCsrHost &h, NodeCsr &d) {
    if (!d.ptr) TRY(dalloc(ctx, &d.ptr, h.ptr.size()));
    if (!d.off) TRY(dalloc(ctx, &d.off, h.off.size()));
    if (!d.stride) TRY(dalloc(ctx, &d.stride, h.stride.size()));
    HIPCHK(hipMemcpyAsync(d.ptr, h.ptr.data(), sizeof(int) * h.ptr.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d.off, h.off.data(), sizeof(long long) * h.off.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d.stride, h.stride.data(), sizeof(int) * h.stride.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}

// the two CSRs of gradient_gather_kernel (0: elastic batches, 1: anchor batches) over the caller's nodes: batch order, then local element
// order, then the element's corners as the caller listed them; built by the first admm_hip_node_forces
static int ensure_gather_csr(admm_hip_ctx *ctx) {
    if (ctx->gr_csr_ready) return ADMM_OK;
    for (int which = 0; which < 2; ++which) {
        std::vector<NodeCsrEntry> entries;
        for (const Batch &b : ctx->batches) {
            if (!energy_evaluated(b) || (b.kind == ADMM_KIND_ANCHOR) != (which == 1)) continue;
            const int nn = ADMM_KIND_NODES[b.kind];
            for (int el = 0; el < b.n_local; ++el) for (int c = 0; c < nn; ++c)
                entries.push_back({b.idx[(size_t)b.local[el] * nn + c], b.gr_cf_off + 3ll * stored_corner(b, b.local[el], c) * b.n_local + el, b.n_local});
        }
        TRY(upload_node_csr(ctx, build_node_csr(ctx->n_nodes, entries), ctx->gr_csr[which]));
    }
    ctx->gr_csr_ready = true;
    return ADMM_OK;
}

// the gradient kernel of one batch on the positions x (device order); stress: also the tets' seven stress values
static int launch_batch_gradient(admm_hip_ctx *ctx, const Batch &b, const double *x, bool stress) {
    return launch_element_kernel(ctx, b, x, admm_dev::GradOut{b.d_escale, b.d_gg, ctx->d_gr_cf + b.gr_cf_off, b.d_gcnt, stress ? b.d_gstress : nullptr, stress ? b.d_gvol : nullptr}, "gradient");
}

// device SoA [rows][n] -> host element-major [n][rows], after the stream has run; the block counts' sum
static int read_gradient_soa(admm_hip_ctx *ctx, const double *dev, int rows, int n, std::vector<double> &tmp) {
    tmp.assign((size_t)rows * std::max(n, 1), 0.0);
    if (n) HIPCHK(hipMemcpyAsync(tmp.data(), dev, sizeof(double) * (size_t)rows * n, hipMemcpyDeviceToHost, ctx->stream));
    return ADMM_OK;
}
static int read_gradient_count(admm_hip_ctx *ctx, const Batch &b, std::vector<int> &cnt) {
    cnt.assign((size_t)std::max(energy_blocks(b.n_local), 1), 0);
    if (b.n_local) HIPCHK(hipMemcpyAsync(cnt.data(), b.d_gcnt, sizeof(int) * (size_t)energy_blocks(b.n_local), hipMemcpyDeviceToHost, ctx->stream));
    return ADMM_OK;
}

int admm_hip_batch_gradient(admm_hip_ctx *ctx, int batch, double *g, double *corner_forces, int64_t *n_nonfinite) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (!energy_evaluated(b)) {      // collision and user-defined batches: not evaluated, zeros
        if (n_nonfinite) *n_nonfinite = 0;
        if (b.kind != ADMM_KIND_GENERIC) {
            if (g) std::fill(g, g + (size_t)b.n_local * ADMM_KIND_ROWS[b.kind], 0.0);
            if (corner_forces) std::fill(corner_forces, corner_forces + (size_t)b.n_local * 3 * ADMM_KIND_NODES[b.kind], 0.0);
        }
        return ADMM_OK;
    }
    TRY(ensure_gradient_buffers(ctx));
    TRY(launch_batch_gradient(ctx, b, ctx->d_x, false));
    const int rows = ADMM_KIND_ROWS[b.kind], nn = ADMM_KIND_NODES[b.kind], n = b.n_local;
    std::vector<double> tg, tc; std::vector<int> cnt;
    TRY(read_gradient_soa(ctx, b.d_gg, rows, n, tg)); TRY(read_gradient_soa(ctx, ctx->d_gr_cf + b.gr_cf_off, 3 * nn, n, tc)); TRY(read_gradient_count(ctx, b, cnt));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    to_element_major(tg, rows, n, g);
    if (corner_forces) for (int el = 0; el < n; ++el) for (int c = 0; c < nn; ++c) {      // the corners as the caller listed them
        const int sc = stored_corner(b, b.local[el], c);
        for (int j = 0; j < 3; ++j) corner_forces[((size_t)el * nn + c) * 3 + j] = tc[(size_t)(3 * sc + j) * n + el];
    }
    if (n_nonfinite) { int64_t t = 0; for (int v : cnt) t += v; *n_nonfinite = t; }
    return ADMM_OK;
}

// parity entry: the same kernel on caller-supplied D_i x rows (element-major [n_local][rows]) instead of the gather, like admm_hip_batch_energy_dx
int admm_hip_batch_gradient_dx(admm_hip_ctx *ctx, int batch, const double *dx, double *g) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size() || !dx) return ADMM_ERR_ARG;
    Batch &b = ctx->batches[batch];
    if (!energy_evaluated(b)) return fail(ctx, ADMM_ERR_UNSUPPORTED, "batch_gradient_dx: no gradient is evaluated for batch %d (kind %d)", batch, b.kind);
    TRY(ensure_gradient_buffers(ctx));
    const int rows = ADMM_KIND_ROWS[b.kind], n = b.n_local;
    if (n == 0) return ADMM_OK;
    std::vector<double> tg;      // (before `supplied`: it is a target of the stream's copies until supplied has waited)
    SuppliedRows supplied(ctx, b);
    TRY(supplied.stage(dx));
    TRY(launch_batch_gradient(ctx, b, ctx->d_x, false));
    if (g) TRY(read_gradient_soa(ctx, b.d_gg, rows, n, tg));
    HIPCHK(supplied.wait());
    to_element_major(tg, rows, n, g);
    return ADMM_OK;
}

int admm_hip_batch_stress(admm_hip_ctx *ctx, int batch, double *stress7, int64_t *n_nonfinite) {
    TRY(require_device(ctx));
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    Batch &b = ctx->batches[batch];
    if (b.kind == ADMM_KIND_GENERIC || !admm_gradient::is_tet(b.kind)) return fail(ctx, ADMM_ERR_UNSUPPORTED, "batch_stress: batch %d (kind %d) is not a tet batch", batch, b.kind);
    TRY(ensure_gradient_buffers(ctx));
    TRY(ensure_stress_buffers(ctx, b));
    TRY(launch_batch_gradient(ctx, b, ctx->d_x, true));
    const int n = b.n_local;
    std::vector<double> ts;
    TRY(read_gradient_soa(ctx, b.d_gstress, 7, n, ts));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    to_element_major(ts, 7, n, stress7);
    int64_t bad = 0;
    for (int el = 0; el < n; ++el) if (!admm_energy::finite(ts[(size_t)6 * n + el])) ++bad;      // (all seven or none: gradient.hpp)
    if (n_nonfinite) *n_nonfinite = bad;
    return ADMM_OK;
}

int admm_hip_node_forces(admm_hip_ctx *ctx, double *f_elastic, double *f_anchor, admm_hip_force_info *info) {
    using namespace admm_dev;
    TRY(require_device(ctx));
    TRY(ensure_gradient_buffers(ctx));
    TRY(ensure_gather_csr(ctx));
    admm_hip_force_info I{};
    std::vector<std::vector<int> > cnt(ctx->batches.size());
    for (size_t bi = 0; bi < ctx->batches.size(); ++bi) {
        const Batch &b = ctx->batches[bi];
        if (!energy_evaluated(b)) { ++I.batches_skipped; continue; }
        TRY(launch_batch_gradient(ctx, b, ctx->d_x, false));
        TRY(read_gradient_count(ctx, b, cnt[bi]));
    }
    const int n = ctx->n_nodes, nblk = energy_blocks(n);
    for (int which = 0; which < 2; ++which) {
        double *host = which ? f_anchor : f_elastic, *dev = ctx->d_gr_out + (size_t)which * 3 * n;
        if (!host || !nblk) continue;
        const NodeCsr &csr = ctx->gr_csr[which];
        hipLaunchKernelGGL(gradient_gather_kernel, dim3(nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, n, (const int *)csr.ptr, (const long long *)csr.off, (const int *)csr.stride, (const double *)ctx->d_gr_cf, dev);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(host, dev, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (const std::vector<int> &c : cnt) for (int v : c) I.n_nonfinite += v;
    if (info) *info = I;
    return ADMM_OK;
}
