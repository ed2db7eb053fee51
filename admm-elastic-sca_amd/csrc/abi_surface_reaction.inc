// abi_surface_reaction.inc -- C ABI: two-way contact, the reaction of a contact on the nodes of the body or sheet surface it landed on
// (kernels_surface_reaction.hpp, surface_reaction.hpp), and the launches admm_hip_step makes for it between its epilogue and the
// velocity damping
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  The launches write v, the feature's own buffers and those of the reaction and attribution
// reports (abi_reaction.inc), nothing else of the solver's state; they run eagerly on the context's stream, outside the captured
// iteration and frame graphs, and drop none of them.  A context whose shares are all zero launches and uploads nothing here.

static bool surface_reaction_any(const admm_hip_ctx *ctx) {
    for (const admm_hip_ctx::CollisionMesh &m : ctx->meshes) if (m.reaction_share > 0.0) return true;
    return false;
}

static int sort_blocks(long long n) { return (int)std::max<long long>((n + admm_dev::SR_BLOCK - 1) / admm_dev::SR_BLOCK, 1); }

// the passes of the stable sort over the first *d_n entries of key / idx [2][half] (half A holds the input): three launches per pass;
// the sorted keys and indices end in half (passes & 1)
static int launch_stable_sort(admm_hip_ctx *ctx, const long long *d_n, int *key, int *idx, size_t half, int nb, int passes, int *blk, int *tot) {
    using namespace admm_dev;
    int *cnt = blk, *off = blk + (size_t)SR_DIGITS * nb;
    for (int p = 0; p < passes; ++p) {
        const int *kin = key + (size_t)(p & 1) * half, *iin = idx + (size_t)(p & 1) * half;
        int *kout = key + (size_t)((p + 1) & 1) * half, *iout = idx + (size_t)((p + 1) & 1) * half;
        hipLaunchKernelGGL(sort_count_kernel, dim3(nb), dim3(SR_BLOCK), 0, ctx->stream, d_n, kin, 8 * p, nb, cnt);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(SR_DIGITS), dim3(RX_SCAN), 0, ctx->stream, d_n, nb, (const int *)cnt, off, tot);
        hipLaunchKernelGGL(sort_place_kernel, dim3(nb), dim3(SR_BLOCK), 0, ctx->stream, d_n, kin, iin, 8 * p, nb, (const int *)off, (const int *)tot, kout, iout);
    }
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// every buffer the frame's launches need, the reaction and attribution reports' included (their first call would otherwise create them
// inside admm_hip_step); a finalized device context with contact attribution on
static int surface_reaction_allocate(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    HIPCHK(hipSetDevice(ctx->device_id));
    if (ctx->sr_ready) return ADMM_OK;
    TRY(attribution_allocate(ctx));
    TRY(ensure_attribution_buffers(ctx));
    const int n = ctx->n_nodes;
    // The capacity.  A contact is a node with depth > depth_min >= 0, and reaction_gather_kernel gives a node without a collision element
    // the depth 0.0 exactly, which is never above depth_min: so K <= the nodes that carry a collision element, whatever the frame.
    // surface_hit_kernel still clamps K to the capacity, as a bound on its writes; were the clamp ever to act, the records would stop
    // short of admm_hip_get_contacts' list -- the invariant above is what rules that out.
    std::vector<char> has((size_t)n, 0);
    for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_COLLISION) for (int el = 0; el < b.n_local; ++el) has[(size_t)b.idx[b.local[el]]] = 1;
    long long cap = 0;
    for (int i = 0; i < n; ++i) cap += has[(size_t)i];
    cap = std::max(cap, 1ll);
    if (3 * cap > 0x7fffffffll - SR_BLOCK) return fail(ctx, ADMM_ERR_ARG, "surface reaction: %lld nodes with a collision element are more than the share tables index", cap);
    ctx->sr_cap = (int)cap; ctx->sr_nb = sort_blocks(3 * cap); ctx->sr_passes = admm_surface_reaction::sort_passes((long long)n + 1);
    const size_t half = 3 * (size_t)cap;
    if (!ctx->d_sr_mesh) {
        std::vector<SrMesh> sm(ctx->meshes.size());
        for (size_t mi = 0; mi < sm.size(); ++mi) {
            const admm_hip_ctx::CollisionMesh &m = ctx->meshes[mi];
            int *vn = nullptr;
            if (m.body()) TRY(upload(ctx, &vn, m.body_nodes));
            sm[mi] = SrMesh{vn, 0.0};
        }
        SrMesh *d = nullptr;
        TRY(upload(ctx, &d, sm));
        ctx->d_sr_mesh = d;
        for (admm_hip_ctx::CollisionMesh &m : ctx->meshes) m.share_dirty = m.reaction_share > 0.0;
    }
    if (!ctx->d_sr_rec) { admm_surface_reaction::Record *r = nullptr; TRY(dalloc(ctx, &r, (size_t)cap)); ctx->d_sr_rec = r; }
    if (!ctx->d_sr_key) TRY(dalloc(ctx, &ctx->d_sr_key, 2 * half));
    if (!ctx->d_sr_idx) TRY(dalloc(ctx, &ctx->d_sr_idx, 2 * half));
    if (!ctx->d_sr_val) TRY(dalloc(ctx, &ctx->d_sr_val, 3 * half));
    if (!ctx->d_sr_blk) TRY(dalloc(ctx, &ctx->d_sr_blk, 2 * (size_t)SR_DIGITS * ctx->sr_nb));
    if (!ctx->d_sr_tot) TRY(dalloc(ctx, &ctx->d_sr_tot, (size_t)SR_DIGITS));
    if (!ctx->d_sr_n) { TRY(dalloc(ctx, &ctx->d_sr_n, 6)); HIPCHK(hipMemset(ctx->d_sr_n, 0, 6 * sizeof(long long))); }      // (the shares' count, then the report's five counts)
    if (!ctx->d_sr_dv) { TRY(dalloc(ctx, &ctx->d_sr_dv, 3 * (size_t)n)); HIPCHK(hipMemset(ctx->d_sr_dv, 0, sizeof(double) * 3 * (size_t)n)); }
    ctx->sr_ready = true;
    return ADMM_OK;
}

// admm_hip_step, directly after epilogue_kernel and before the damping filter, while some share is above zero
static int launch_surface_reaction(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    if (!ctx->sr_ready) return fail(ctx, ADMM_ERR_STATE, "surface reaction: a share is set but the buffers were never allocated");
    const double depth_min = ctx->sr_depth_min;
    const int n = ctx->n_nodes, cap = ctx->sr_cap, nb = ctx->sr_nb, passes = ctx->sr_passes;
    const size_t half = 3 * (size_t)cap;
    SrMesh *sm = (SrMesh *)ctx->d_sr_mesh;
    for (size_t mi = 0; mi < ctx->meshes.size(); ++mi) {      // (the shares travel as kernel arguments: no host buffer has to outlive the call)
        admm_hip_ctx::CollisionMesh &m = ctx->meshes[mi];
        if (!m.share_dirty) continue;
        hipLaunchKernelGGL(surface_share_kernel, dim3(1), dim3(SR_BLOCK), 0, ctx->stream, sm, (int)mi, m.reaction_share);
        m.share_dirty = false;
    }
    int *skey = ctx->d_sr_key + (size_t)(passes & 1) * half, *sidx = ctx->d_sr_idx + (size_t)(passes & 1) * half;
    // the nodes the last reacting frame wrote go back to 0.0 (its sorted keys and their count are still in place)
    hipLaunchKernelGGL(surface_clear_kernel, dim3(nb), dim3(SR_BLOCK), 0, ctx->stream, (const long long *)ctx->d_sr_n, (const int *)skey, n, ctx->d_sr_dv);
    HIPCHK(hipGetLastError());
    // the contacts of admm_hip_get_contacts(depth_min) and their owners, by the reports' own launches
    TRY(launch_contact_chain(ctx, depth_min, CHAIN_RECORDS | CHAIN_OWNERS));
    hipLaunchKernelGGL(surface_hit_kernel, dim3((cap + SR_BLOCK - 1) / SR_BLOCK), dim3(SR_BLOCK), 0, ctx->stream, (const long long *)ctx->d_rx_count, (const ContactRecord *)ctx->d_rx_rec,
                       (const OwnerRecord *)ctx->d_at_rec, (const ShapeTable *)ctx->d_shapes, (const admm_mesh::MeshDev *)ctx->d_meshes,
                       (const admm_mesh::MeshMotion *)ctx->d_mesh_motion, (const SrMesh *)sm, (const int *)ctx->d_body_tag, (const int *)ctx->d_iperm, ctx->dt, n, (long long)cap,
                       (admm_surface_reaction::Record *)ctx->d_sr_rec, ctx->d_sr_key, ctx->d_sr_idx, ctx->d_sr_val, ctx->d_sr_n);
    HIPCHK(hipGetLastError());
    TRY(launch_stable_sort(ctx, ctx->d_sr_n, ctx->d_sr_key, ctx->d_sr_idx, half, nb, passes, ctx->d_sr_blk, ctx->d_sr_tot));
    hipLaunchKernelGGL(surface_apply_kernel, dim3(nb), dim3(SR_BLOCK), 0, ctx->stream, (const long long *)ctx->d_sr_n, (const int *)skey, (const int *)sidx, (const double *)ctx->d_sr_val, n,
                       (const int *)ctx->d_iperm, (const double *)ctx->d_m3, ctx->d_v, ctx->d_sr_dv);
    HIPCHK(hipGetLastError());
    ctx->sr_frame = ctx->frames;
    return ADMM_OK;
}

int admm_hip_set_surface_reaction(admm_hip_ctx *ctx, int mesh_id, double share) {
    if (!ctx) return ADMM_ERR_ARG;
    admm_hip_ctx::CollisionMesh *m = mesh_by_id(ctx, mesh_id);
    if (!m) return ADMM_ERR_ARG;
    if (!m->body()) return fail(ctx, ADMM_ERR_ARG, "set_surface_reaction: collision mesh %d is an obstacle, not a body or sheet surface: its vertices are no simulated nodes", mesh_id);
    if (!(share >= 0.0 && share <= 1.0)) return fail(ctx, ADMM_ERR_ARG, "set_surface_reaction: mesh %d: share %g lies outside [0, 1]", mesh_id, share);
    if (share > 0.0 && !ctx->attribution)
        return fail(ctx, ADMM_ERR_STATE, "set_surface_reaction: mesh %d: contact attribution is off (admm_hip_enable_contact_attribution): a reaction needs every contact's owner entry", mesh_id);
    if (share > 0.0 && ctx->world > 1)
        return fail(ctx, ADMM_ERR_UNSUPPORTED, "set_surface_reaction: mesh %d: not available in a sharded context (world = %d): a destination node may live on another rank", mesh_id, ctx->world);
    if (share > 0.0 && ctx->finalized && ctx->device_id >= 0) TRY(surface_reaction_allocate(ctx));      // (before finalize: finalize does it)
    if (share != m->reaction_share) m->share_dirty = true;      // (reaches the device with the next step's launches)
    m->reaction_share = share;
    return ADMM_OK;
}

int admm_hip_set_surface_reaction_depth(admm_hip_ctx *ctx, double depth_min) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!(depth_min >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "set_surface_reaction_depth: depth_min must be >= 0, got %g", depth_min);
    ctx->sr_depth_min = depth_min;
    return ADMM_OK;
}

int admm_hip_get_surface_reaction(admm_hip_ctx *ctx, double *dv, admm_hip_surface_contact *records, int64_t capacity, int64_t *count, admm_hip_surface_reaction_info *info) {
    if (!ctx) return ADMM_ERR_ARG;
    if (capacity < 0 || (capacity && !records)) return fail(ctx, ADMM_ERR_ARG, "get_surface_reaction: capacity must be >= 0 and records given with it");
    TRY(require_reactions(ctx, "get_surface_reaction"));
    const size_t n = (size_t)ctx->n_nodes;
    admm_hip_surface_reaction_info I{};
    if (ctx->sr_frame != ctx->frames || !ctx->sr_ready) {      // the last frame ran no reaction: nothing landed anywhere
        if (dv) std::fill(dv, dv + 3 * n, 0.0);
        if (count) *count = 0;
        if (info) *info = I;
        return ADMM_OK;
    }
    HIPCHK(hipSetDevice(ctx->device_id));
    static_assert(sizeof(admm_hip_surface_contact) == sizeof(admm_surface_reaction::Record), "admm_hip_surface_contact is the device's record");
    static_assert(sizeof(admm_hip_surface_reaction_info) == 5 * sizeof(long long), "the info is the five counts surface_info_kernel writes");
    // the counts by status are summed on the device; the records that fit the caller's capacity follow once their number is known
    // (a second, short wait in place of a copy of every record the buffer could hold)
    long long h[6] = {0, 0, 0, 0, 0, 0};
    hipLaunchKernelGGL(admm_dev::surface_info_kernel, dim3(1), dim3(admm_dev::SR_BLOCK), 0, ctx->stream, (const long long *)ctx->d_sr_n,
                       (const admm_surface_reaction::Record *)ctx->d_sr_rec, ctx->d_sr_n + 1);
    HIPCHK(hipGetLastError());
    if (dv) HIPCHK(hipMemcpyAsync(dv, ctx->d_sr_dv, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h, ctx->d_sr_n, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const long long K = h[0] / 3;
    I.n_contacts = h[1]; I.n_reacting = h[2]; I.n_unowned = h[3]; I.n_other = h[4]; I.n_self = h[5];
    const size_t got = (size_t)std::min<long long>(std::min<long long>(K, capacity), ctx->sr_cap);
    if (got) {
        HIPCHK(hipMemcpyAsync(records, ctx->d_sr_rec, sizeof(admm_hip_surface_contact) * got, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (count) *count = K;
    if (info) *info = I;
    return ADMM_OK;
}

// the feature's sort kernels alone: perm [n] = the stable order of keys [n], every key in [0, key_bound)
int admm_hip_debug_stable_sort(admm_hip_ctx *ctx, int64_t n, const int32_t *keys, int64_t key_bound, int32_t *perm) {
    using namespace admm_dev;
    if (!ctx) return ADMM_ERR_ARG;
    if (n < 0 || n > 0x7fffffffll - SR_BLOCK || key_bound < 1 || key_bound > 0x7fffffffll || (n && (!keys || !perm)))
        return fail(ctx, ADMM_ERR_ARG, "debug_stable_sort: n %lld or key_bound %lld out of range, or keys / perm missing", (long long)n, (long long)key_bound);
    for (int64_t i = 0; i < n; ++i) if (keys[i] < 0 || keys[i] >= key_bound) return fail(ctx, ADMM_ERR_ARG, "debug_stable_sort: key %lld is %d, outside [0, %lld)", (long long)i, (int)keys[i], (long long)key_bound);
    TRY(require_device(ctx));
    HIPCHK(hipSetDevice(ctx->device_id));
    const int nb = sort_blocks(n), passes = admm_surface_reaction::sort_passes(key_bound);
    const size_t half = (size_t)std::max<int64_t>(n, 1);
    int *buf = nullptr; long long *dn = nullptr;      // key [2][half], idx [2][half], counts and offsets [2][256][nb], totals [256]
    const size_t ints = 4 * half + 2 * (size_t)SR_DIGITS * nb + SR_DIGITS;
    HIPCHK(hipMalloc((void **)&buf, sizeof(int) * ints));
    if (hipMalloc((void **)&dn, sizeof(long long)) != hipSuccess) { (void)hipFree(buf); (void)hipGetLastError(); return fail(ctx, ADMM_ERR_HIP, "debug_stable_sort: hipMalloc failed"); }
    int *key = buf, *idx = buf + 2 * half, *blk = buf + 4 * half, *tot = blk + 2 * (size_t)SR_DIGITS * nb;
    const long long nn = n;
    int rc = ADMM_OK;
    hipError_t e = hipMemcpyAsync(dn, &nn, sizeof nn, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(key, keys, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sort_iota_kernel, dim3(nb), dim3(SR_BLOCK), 0, ctx->stream, (const long long *)dn, idx);
        rc = launch_stable_sort(ctx, dn, key, idx, half, nb, passes, blk, tot);
        if (!rc && n) e = hipMemcpyAsync(perm, idx + (size_t)(passes & 1) * half, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    (void)hipFree(buf); (void)hipFree(dn);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) { (void)hipGetLastError(); return fail(ctx, ADMM_ERR_HIP, "debug_stable_sort: %s", hipGetErrorString(e != hipSuccess ? e : es)); }
    return ADMM_OK;
}
