// abi_attach.inc -- C ABI: rigid attachments, whole ANCHOR batches fastened to rigid bodies (kernels_attach.hpp, attach.hpp), and the two
// launches abi_rigid.inc's hooks make for them: the targets behind the pose at the very start of admm_hip_step, the load before the
// bodies' integration
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  The launches write the attached batches' targets, the attachment rows and the bodies' rows of
// d_rg_out, nothing else; they run eagerly on the context's stream, outside the captured iteration and frame graphs, and drop none of
// them (a batch's targets keep their address).  A context without an attached batch launches and uploads nothing here.

static bool attach_any(const admm_hip_ctx *ctx) {
    for (const Batch &b : ctx->batches) if (b.attach_body >= 0) return true;
    return false;
}

// every buffer the launches need, sized for every anchor batch the context has, and the tables of the attachments as the host holds
// them; a finalized device context (or finalize itself).  The frames queued so far read the tables as they were.
static int attach_upload(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    HIPCHK(hipSetDevice(ctx->device_id));
    if (!ctx->att_ready) {
        size_t slots = 0, elems = 0, blocks = 0;
        for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_ANCHOR) { ++slots; elems += (size_t)b.n_local; blocks += (size_t)energy_blocks(b.n_local); }
        ctx->att_pcap = (int)blocks + ADMM_MAX_SHAPES;
        if (!ctx->d_att_bat) { AttachBatchDev *p = nullptr; TRY(dalloc(ctx, &p, slots)); ctx->d_att_bat = p; }
        if (!ctx->d_att_blk) { AttachBlock *p = nullptr; TRY(dalloc(ctx, &p, blocks)); ctx->d_att_blk = p; }
        if (!ctx->d_att_slot) TRY(dalloc(ctx, &ctx->d_att_slot, elems));
        if (!ctx->d_att_elem) TRY(dalloc(ctx, &ctx->d_att_elem, elems));
        if (!ctx->d_att_total) TRY(dalloc(ctx, &ctx->d_att_total, (size_t)ADMM_MAX_SHAPES));
        if (!ctx->d_att_carry) TRY(dalloc(ctx, &ctx->d_att_carry, (size_t)ADMM_MAX_SHAPES));
        if (!ctx->d_att_part) TRY(dalloc(ctx, &ctx->d_att_part, 6 * (size_t)ctx->att_pcap));
        if (!ctx->d_att_cnt) TRY(dalloc(ctx, &ctx->d_att_cnt, (size_t)ctx->att_pcap));
        if (!ctx->d_att_out) { TRY(dalloc(ctx, &ctx->d_att_out, 6 * (size_t)ADMM_MAX_SHAPES)); HIPCHK(hipMemset(ctx->d_att_out, 0, sizeof(double) * 6 * ADMM_MAX_SHAPES)); }
        if (!ctx->d_att_nact) { TRY(dalloc(ctx, &ctx->d_att_nact, (size_t)ADMM_MAX_SHAPES)); HIPCHK(hipMemset(ctx->d_att_nact, 0, sizeof(long long) * ADMM_MAX_SHAPES)); }
        ctx->att_ready = true;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<AttachBatchDev> bat; std::vector<AttachBlock> blk;
    std::vector<int> slot_of(ctx->batches.size(), -1), carry(ADMM_MAX_SHAPES, 0);
    std::vector<long long> total(ADMM_MAX_SHAPES, 0);
    for (size_t k = 0; k < ctx->batches.size(); ++k) {
        Batch &b = ctx->batches[k];
        if (b.attach_body < 0) continue;
        const int nl = b.n_local;
        if (!b.d_attach_local) TRY(dalloc(ctx, &b.d_attach_local, 3 * (size_t)nl));
        std::vector<double> loc(3 * (size_t)std::max(nl, 1), 0.0);
        for (int el = 0; el < nl; ++el) for (int j = 0; j < 3; ++j) loc[3 * (size_t)el + j] = b.attach_local[3 * (size_t)b.local[el] + j];
        if (nl) HIPCHK(hipMemcpy(b.d_attach_local, loc.data(), sizeof(double) * 3 * (size_t)nl, hipMemcpyHostToDevice));
        slot_of[k] = (int)bat.size();
        bat.push_back(AttachBatchDev{b.d_idx, b.d_w2, b.d_active, b.d_u, b.d_z, b.d_targets, b.d_attach_local, nl, b.attach_body});
        for (int first = 0; first < nl; first += ENERGY_BLOCK) blk.push_back(AttachBlock{slot_of[k], first});
        carry[b.attach_body] = 1; total[b.attach_body] += nl;
    }
    std::vector<int> el_slot, el_elem;      // sorted by (body, batch index, element)
    for (int body = 0; body < (int)ctx->rigid.size(); ++body) {
        for (size_t k = 0; k < ctx->batches.size(); ++k) if (ctx->batches[k].attach_body == body)
            for (int el = 0; el < ctx->batches[k].n_local; ++el) { el_slot.push_back(slot_of[k]); el_elem.push_back(el); }
    }
    const int pblk = (int)admm_layout::blocks_before(total.data(), (int)ctx->rigid.size());      // the blocks of all bodies
    if (pblk > ctx->att_pcap) return fail(ctx, ADMM_ERR_STATE, "attachments: %d blocks of attached elements, room for %d", pblk, ctx->att_pcap);
    if (!bat.empty()) HIPCHK(hipMemcpy(ctx->d_att_bat, bat.data(), sizeof(AttachBatchDev) * bat.size(), hipMemcpyHostToDevice));
    if (!blk.empty()) HIPCHK(hipMemcpy(ctx->d_att_blk, blk.data(), sizeof(AttachBlock) * blk.size(), hipMemcpyHostToDevice));
    if (!el_slot.empty()) {
        HIPCHK(hipMemcpy(ctx->d_att_slot, el_slot.data(), sizeof(int) * el_slot.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ctx->d_att_elem, el_elem.data(), sizeof(int) * el_elem.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(ctx->d_att_total, total.data(), sizeof(long long) * total.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_att_carry, carry.data(), sizeof(int) * carry.size(), hipMemcpyHostToDevice));
    if (bat.empty()) {      // the last batch went: the rows read as no load
        HIPCHK(hipMemset(ctx->d_att_out, 0, sizeof(double) * 6 * ADMM_MAX_SHAPES));
        HIPCHK(hipMemset(ctx->d_att_nact, 0, sizeof(long long) * ADMM_MAX_SHAPES));
    }
    ctx->att_slots = (int)bat.size(); ctx->att_tblk = (int)blk.size(); ctx->att_pblk = pblk;
    return ADMM_OK;
}

// launch_rigid_pose, behind rigid_pose_kernel: the attached batches' targets from the bodies' records, before anything reads a target
static int launch_attach_targets(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    if (!ctx->att_slots || !ctx->att_tblk) return ADMM_OK;
    hipLaunchKernelGGL(attach_targets_kernel, dim3(ctx->att_tblk), dim3(ENERGY_BLOCK), 0, ctx->stream, (const AttachBlock *)ctx->d_att_blk, (const AttachBatchDev *)ctx->d_att_bat, ctx->att_slots,
                       (int)ctx->rigid.size(), (const admm_rigid::Record *)ctx->d_rg_rec);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// launch_rigid_integrate, behind rigid_reduce_kernel and before rigid_integrate_kernel: the attachment rows, added to the contacts' rows
static int launch_attach_load(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    if (!ctx->att_slots) return ADMM_OK;
    const int nb = (int)ctx->rigid.size(), n_part = std::max(ctx->att_pblk, 1);
    if (ctx->att_pblk)
        hipLaunchKernelGGL(attach_partial_kernel, dim3(ctx->att_pblk), dim3(ENERGY_BLOCK), 0, ctx->stream, (const int *)ctx->d_att_slot, (const int *)ctx->d_att_elem,
                           (const AttachBatchDev *)ctx->d_att_bat, ctx->att_slots, nb, (const long long *)ctx->d_att_total, (const admm_rigid::Record *)ctx->d_rg_rec, (const double *)ctx->d_x,
                           n_part, ctx->d_att_part, ctx->d_att_cnt);
    hipLaunchKernelGGL(attach_reduce_kernel, dim3(6 * nb), dim3(ENERGY_REDUCE), 0, ctx->stream, (const long long *)ctx->d_att_total, (const int *)ctx->d_att_carry, n_part,
                       (const double *)ctx->d_att_part, (const int *)ctx->d_att_cnt, ctx->d_att_out, ctx->d_att_nact, ctx->d_rg_out);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// the batch's targets as the device holds them now, into the host's copy (one synchronisation); a host-only or unfinalized context keeps its own
static int attach_fetch_targets(admm_hip_ctx *ctx, Batch &b) {
    if (!ctx->finalized || ctx->device_id < 0 || !b.n_local) return ADMM_OK;
    HIPCHK(hipSetDevice(ctx->device_id));
    std::vector<double> t(3 * (size_t)b.n_local);
    HIPCHK(hipMemcpyAsync(t.data(), b.d_targets, sizeof(double) * t.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int el = 0; el < b.n_local; ++el) for (int j = 0; j < 3; ++j) b.targets[3 * (size_t)b.local[el] + j] = t[3 * (size_t)el + j];
    return ADMM_OK;
}

static Batch *attach_anchor_batch(admm_hip_ctx *ctx, int batch, const char *who) {
    if (batch >= 0 && batch < (int)ctx->batches.size() && ctx->batches[batch].kind == ADMM_KIND_ANCHOR) return &ctx->batches[batch];
    fail(ctx, ADMM_ERR_ARG, "%s: batch %d is not an anchor batch (have %d batches)", who, batch, (int)ctx->batches.size());
    return nullptr;
}

int admm_hip_attach_anchors(admm_hip_ctx *ctx, int batch, int body, const double *local) {
    if (!ctx) return ADMM_ERR_ARG;
    Batch *bp = attach_anchor_batch(ctx, batch, "attach_anchors");
    if (!bp) return ADMM_ERR_ARG;
    Batch &b = *bp;
    if (body < 0 || body >= (int)ctx->rigid.size()) return fail(ctx, ADMM_ERR_ARG, "attach_anchors: body %d is not a rigid body (have %d)", body, (int)ctx->rigid.size());
    if (b.attach_body >= 0) return fail(ctx, ADMM_ERR_ARG, "attach_anchors: batch %d is attached already (to body %d): detach it first", batch, b.attach_body);
    const size_t n3 = 3 * (size_t)b.n_total;
    if (local) for (size_t i = 0; i < n3; ++i) if (!std::isfinite(local[i]))
        return fail(ctx, ADMM_ERR_ARG, "attach_anchors: batch %d: the offset of element %d is not finite", batch, (int)(i / 3));
    if (ctx->world > 1)
        return fail(ctx, ADMM_ERR_UNSUPPORTED, "attach_anchors: batch %d: not available in a sharded context (world = %d): a rank holds only its share of the batch", batch, ctx->world);
    std::vector<double> off(n3);
    if (local) std::copy(local, local + n3, off.begin());
    else {      // from the batch's current targets and the body's current pose
        admm_rigid::Record R = ctx->rigid[body].rec;
        if (ctx->rg_ready) {
            HIPCHK(hipSetDevice(ctx->device_id));
            HIPCHK(hipMemcpyAsync(&R, (const admm_rigid::Record *)ctx->d_rg_rec + body, sizeof R, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        TRY(attach_fetch_targets(ctx, b));
        for (int e = 0; e < b.n_total; ++e) {
            // (a static batch's targets are its nodes' positions, which the host fills in at finalize)
            const double *t = (!ctx->finalized && !b.moving) ? &ctx->x[3 * (size_t)b.idx[e]] : &b.targets[3 * (size_t)e];
            admm_attach::local_offset(R.c, R.R, t, &off[3 * (size_t)e]);
        }
        for (size_t i = 0; i < n3; ++i) if (!std::isfinite(off[i]))
            return fail(ctx, ADMM_ERR_ARG, "attach_anchors: batch %d: the offset of element %d, derived from its target, is not finite", batch, (int)(i / 3));
    }
    b.attach_local.swap(off); b.attach_body = body;
    if (ctx->finalized && ctx->device_id >= 0) {      // (before finalize: finalize does it)
        const int rc = attach_upload(ctx);
        if (rc) { b.attach_body = -1; b.attach_local.clear(); return rc; }
    }
    return ADMM_OK;
}

int admm_hip_detach_anchors(admm_hip_ctx *ctx, int batch) {
    if (!ctx) return ADMM_ERR_ARG;
    Batch *bp = attach_anchor_batch(ctx, batch, "detach_anchors");
    if (!bp) return ADMM_ERR_ARG;
    if (bp->attach_body < 0) return fail(ctx, ADMM_ERR_ARG, "detach_anchors: batch %d is not attached", batch);
    TRY(attach_fetch_targets(ctx, *bp));      // the targets stay where the last frame put them, on the host's side too
    bp->attach_body = -1; bp->attach_local.clear();
    if (ctx->finalized && ctx->device_id >= 0) TRY(attach_upload(ctx));
    return ADMM_OK;
}

int admm_hip_get_attachment(admm_hip_ctx *ctx, int batch, int *body, double *local, double *targets) {
    if (!ctx) return ADMM_ERR_ARG;
    Batch *bp = attach_anchor_batch(ctx, batch, "get_attachment");
    if (!bp) return ADMM_ERR_ARG;
    Batch &b = *bp;
    if (body) *body = b.attach_body;
    const size_t n3 = 3 * (size_t)b.n_total;
    if (local) { if (b.attach_body >= 0) std::copy(b.attach_local.begin(), b.attach_local.end(), local); else std::fill(local, local + n3, 0.0); }
    if (targets) { TRY(attach_fetch_targets(ctx, b)); std::copy(b.targets.begin(), b.targets.end(), targets); }
    return ADMM_OK;
}

int admm_hip_get_attachment_load(admm_hip_ctx *ctx, int n_bodies, double *Fa, double *Ta, int64_t *n_active) {
    if (!ctx) return ADMM_ERR_ARG;
    if (n_bodies != (int)ctx->rigid.size()) return fail(ctx, ADMM_ERR_ARG, "get_attachment_load: %d rows given, the context has %d rigid bodies", n_bodies, (int)ctx->rigid.size());
    std::vector<double> h(6 * (size_t)std::max(n_bodies, 1), 0.0); std::vector<long long> c((size_t)std::max(n_bodies, 1), 0);
    if (n_bodies && ctx->att_ready) {
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipMemcpyAsync(h.data(), ctx->d_att_out, sizeof(double) * 6 * (size_t)n_bodies, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(c.data(), ctx->d_att_nact, sizeof(long long) * (size_t)n_bodies, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    for (int b = 0; b < n_bodies; ++b) {
        for (int j = 0; j < 3; ++j) { if (Fa) Fa[3 * (size_t)b + j] = h[6 * (size_t)b + j]; if (Ta) Ta[3 * (size_t)b + j] = h[6 * (size_t)b + 3 + j]; }
        if (n_active) n_active[b] = c[b];
    }
    return ADMM_OK;
}
