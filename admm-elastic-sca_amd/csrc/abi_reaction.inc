// abi_reaction.inc -- C ABI: the reactions of the one-node constraints (COLLISION, ANCHOR) in the last frame, per element and per node,
// the compact list of the nodes in contact and their resultant (kernels_reaction.hpp, reaction.hpp); contact attribution (attribution.hpp):
// the switch, the owner entry and normal per element and per contact, the per-entry resultants
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  Nothing here writes x, v, u, z, the warm starts, the cost counters or the sides, and nothing
// drops a captured graph: the kernels read the state and write buffers of their own.  Every launch and copy is asynchronous on the
// context's stream, which the call then waits for once (DESIGN.md section 7, "Streams").

static bool reaction_reported(const Batch &b) { return b.kind == ADMM_KIND_COLLISION || b.kind == ADMM_KIND_ANCHOR; }
static int reaction_blocks(int n) { return (n + admm_dev::RX_BLOCK - 1) / admm_dev::RX_BLOCK; }

// what every entry checks after its own arguments: a device context with a usable factor that has stepped at least once
static int require_reactions(admm_hip_ctx *ctx, const char *who) {
    TRY(require_factor(ctx));
    if (ctx->frames == 0) return fail(ctx, ADMM_ERR_STATE, "%s: no frame has run yet: a reaction is that of the last admm_hip_step", who);
    return ADMM_OK;
}

// the buffers of the two-stage row sums behind the chain (kernels_reaction.hpp: entry_partial_kernel / entry_reduce_kernel and their
// rigid twins): rows rows, row q's contacts perm[sum of totals before q ...) (null: the records in order), counts / offsets
// [rows_max][nblk] for the sort, partials [6][n_part], out [rows][6].  sorted: the entries' rows + one for the contacts without an owner,
// on the attribution reports' buffers; else one row, all contacts, on buffers that exist without attribution
struct EntryWork { int *counts, *offsets; long long *totals; int *perm; double *partials, *out; int nblk, n_part, rows; };
static EntryWork entry_work(const admm_hip_ctx *ctx, bool sorted) {
    const long long items = std::max(ctx->n_nodes, 1);
    const int rows_max = sorted ? ADMM_MAX_SHAPES + 1 : 1, nblk = (int)admm_layout::row_blocks(items), n_part = (int)admm_layout::partial_blocks_bound(items, rows_max);
    if (!sorted) return EntryWork{nullptr, nullptr, ctx->d_rx_count, nullptr, ctx->d_rx_part, ctx->d_rx_part + 6 * (size_t)n_part, nblk, n_part, 1};
    return EntryWork{ctx->d_at_blk, ctx->d_at_blk + (size_t)rows_max * nblk, ctx->d_at_tot, ctx->d_at_perm, ctx->d_at_part, ctx->d_at_out, nblk, n_part, ctx->shapes.n + 1};
}

// every buffer the kernels write and the gather's two CSRs (0: the collision batches, 1: the anchor batches; batch order, then local
// element order), created by the first call
static int ensure_reaction_buffers(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    HIPCHK(hipSetDevice(ctx->device_id));
    if (ctx->rx_ready) return ADMM_OK;
    const int n = ctx->n_nodes;
    long long total = 0;      // (what a call that failed further down allocated is reused: the sizes depend on the scene alone)
    for (Batch &b : ctx->batches) {
        if (!reaction_reported(b)) continue;
        b.rx_off = total;
        total += (long long)RX_ROWS * std::max(b.n_local, 1);
    }
    if (!ctx->d_rx_el) TRY(dalloc(ctx, &ctx->d_rx_el, (size_t)std::max(total, 1ll)));
    if (!ctx->d_rx_node) TRY(dalloc(ctx, &ctx->d_rx_node, 10 * (size_t)std::max(n, 1)));
    if (!ctx->d_rx_blk) TRY(dalloc(ctx, &ctx->d_rx_blk, 2 * (size_t)std::max(reaction_blocks(n), 1)));
    if (!ctx->d_rx_count) TRY(dalloc(ctx, &ctx->d_rx_count, 1));
    if (!ctx->d_rx_rec) { ContactRecord *r = nullptr; TRY(dalloc(ctx, &r, (size_t)std::max(n, 1))); ctx->d_rx_rec = r; }
    if (!ctx->d_rx_part) TRY(dalloc(ctx, &ctx->d_rx_part, 6 * (size_t)entry_work(ctx, false).n_part + 6));
    for (int which = 0; which < 2; ++which) {
        const int kind = which ? ADMM_KIND_ANCHOR : ADMM_KIND_COLLISION;
        std::vector<NodeCsrEntry> entries;
        for (const Batch &b : ctx->batches) if (b.kind == kind)
            for (int el = 0; el < b.n_local; ++el) entries.push_back({b.idx[b.local[el]], b.rx_off + el, b.n_local});
        TRY(upload_node_csr(ctx, build_node_csr(n, entries), ctx->rx_csr[which]));
    }
    ctx->rx_ready = true;
    return ADMM_OK;
}

// the per-element kernel of one batch: seven rows at rx_off of d_rx_el
static int launch_batch_reaction(admm_hip_ctx *ctx, const Batch &b) {
    using namespace admm_dev;
    const int nblk = energy_blocks(b.n_local);
    if (nblk) hipLaunchKernelGGL(reaction_elem_kernel, dim3(nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, b.n_local, (const int *)b.d_idx, (const double *)b.d_w2, (const double *)b.d_u,
                                 (const double *)b.d_z, (const double *)ctx->d_x, ctx->d_rx_el + b.rx_off);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// The contact chain, the one launch sequence behind every report and feature that reads the contacts of the last frame.  Always: every
// reported batch's elements, the nodes' sums, depths and points -> d_rx_node, and the count and scan of the nodes with depth > depth_min
// (the count stays on the device, at d_rx_count).  Then what `what` asks for, in this order: CHAIN_RECORDS the contact records -> d_rx_rec;
// CHAIN_OWNERS the owner records of the same contacts in the same places -> d_at_rec; CHAIN_SORTED (with CHAIN_OWNERS) the contacts
// sorted by entry: entry_count / row_scan / entry_place -> entry_work(ctx, true).  The last two need ensure_attribution_buffers.
// Every caller runs the whole chain with its own depth_min; nothing is kept from one call to the next.
enum { CHAIN_NODES = 0, CHAIN_RECORDS = 1, CHAIN_OWNERS = 2, CHAIN_SORTED = 4 };

static int launch_contact_chain(admm_hip_ctx *ctx, double depth_min, int what, admm_hip_reaction_info *info = nullptr) {
    using namespace admm_dev;
    for (const Batch &b : ctx->batches) {
        if (!reaction_reported(b)) { if (info) ++info->batches_skipped; continue; }
        if (info) ++(b.kind == ADMM_KIND_ANCHOR ? info->batches_anchor : info->batches_collision);
        TRY(launch_batch_reaction(ctx, b));
    }
    const int n = ctx->n_nodes, gblk = energy_blocks(n), nblk = reaction_blocks(n);
    const NodeCsr &cc = ctx->rx_csr[0], &ca = ctx->rx_csr[1];
    if (gblk) hipLaunchKernelGGL(reaction_gather_kernel, dim3(gblk), dim3(ENERGY_BLOCK), 0, ctx->stream, n, (const int *)cc.ptr, (const long long *)cc.off, (const int *)cc.stride,
                                 (const int *)ca.ptr, (const long long *)ca.off, (const int *)ca.stride, (const double *)ctx->d_rx_el, ctx->d_rx_node);
    int *cnt = ctx->d_rx_blk, *off = ctx->d_rx_blk + std::max(nblk, 1);
    const double *nodes = ctx->d_rx_node;
    if (nblk) hipLaunchKernelGGL(contact_count_kernel, dim3(nblk), dim3(RX_BLOCK), 0, ctx->stream, n, nodes + 6 * (size_t)n, depth_min, cnt);
    hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(RX_SCAN), 0, ctx->stream, nblk, (const int *)cnt, off, ctx->d_rx_count);
    if ((what & CHAIN_RECORDS) && nblk)
        hipLaunchKernelGGL(contact_scatter_kernel, dim3(nblk), dim3(RX_BLOCK), 0, ctx->stream, n, nodes, depth_min, (const int *)off, (long long)n, (ContactRecord *)ctx->d_rx_rec);
    if ((what & CHAIN_OWNERS) && nblk)
        hipLaunchKernelGGL(contact_owner_scatter_kernel, dim3(nblk), dim3(RX_BLOCK), 0, ctx->stream, n, nodes, depth_min, (const int *)off, (long long)n, (const int *)cc.ptr,
                           (const long long *)cc.off, (const int *)cc.stride, (const long long *)ctx->d_at_csr, (const double *)ctx->d_rx_el, (const int *)ctx->d_at_owner,
                           (const double *)ctx->d_at_normal, ctx->at_total, (OwnerRecord *)ctx->d_at_rec);
    if (what & CHAIN_SORTED) {
        const EntryWork W = entry_work(ctx, true);
        const long long *count = ctx->d_rx_count;
        const OwnerRecord *orec = (const OwnerRecord *)ctx->d_at_rec;
        hipLaunchKernelGGL(entry_count_kernel, dim3(W.nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, count, orec, W.rows, W.nblk, W.counts);
        hipLaunchKernelGGL(row_scan_kernel, dim3(W.rows), dim3(RX_SCAN), 0, ctx->stream, W.nblk, (const int *)W.counts, W.offsets, W.totals);
        hipLaunchKernelGGL(entry_place_kernel, dim3(W.nblk), dim3(ENERGY_BLOCK), 0, ctx->stream, count, orec, W.rows, W.nblk, (const int *)W.offsets, (const long long *)W.totals, W.perm);
    }
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// behind the chain: W's rows about one pivot (null: the origin), entry_partial_kernel then entry_reduce_kernel -> W.out [rows][6]
static int launch_row_sums(admm_hip_ctx *ctx, const EntryWork &W, const double *pivot) {
    using namespace admm_dev;
    const double p0 = pivot ? pivot[0] : 0.0, p1 = pivot ? pivot[1] : 0.0, p2 = pivot ? pivot[2] : 0.0;
    hipLaunchKernelGGL(entry_partial_kernel, dim3(W.nblk + W.rows), dim3(ENERGY_BLOCK), 0, ctx->stream, (const ContactRecord *)ctx->d_rx_rec, (const int *)W.perm, W.rows, (const long long *)W.totals, p0, p1, p2,
                       W.n_part, W.partials);
    hipLaunchKernelGGL(entry_reduce_kernel, dim3(6 * W.rows), dim3(ENERGY_REDUCE), 0, ctx->stream, W.rows, (const long long *)W.totals, W.n_part, (const double *)W.partials, W.out);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

int admm_hip_batch_reaction(admm_hip_ctx *ctx, int batch, double *f, double *depth) {
    if (!ctx) return ADMM_ERR_ARG;
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (!reaction_reported(b)) return fail(ctx, ADMM_ERR_UNSUPPORTED, "batch_reaction: batch %d (kind %d) is neither a collision nor an anchor batch", batch, b.kind);
    TRY(require_reactions(ctx, "batch_reaction"));
    TRY(ensure_reaction_buffers(ctx));
    TRY(launch_batch_reaction(ctx, b));
    const int n = b.n_local;
    std::vector<double> t(4 * (size_t)std::max(n, 1), 0.0);
    if (n) HIPCHK(hipMemcpyAsync(t.data(), ctx->d_rx_el + b.rx_off, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int el = 0; el < n; ++el) {
        if (f) for (int j = 0; j < 3; ++j) f[3 * (size_t)el + j] = t[(size_t)j * n + el];
        if (depth) depth[el] = t[(size_t)3 * n + el];
    }
    return ADMM_OK;
}

int admm_hip_node_reactions(admm_hip_ctx *ctx, double *f_contact, double *f_anchor, admm_hip_reaction_info *info) {
    if (!ctx) return ADMM_ERR_ARG;
    TRY(require_reactions(ctx, "node_reactions"));
    TRY(ensure_reaction_buffers(ctx));
    admm_hip_reaction_info I{};
    TRY(launch_contact_chain(ctx, 0.0, CHAIN_NODES, &I));
    const size_t n = (size_t)ctx->n_nodes;
    long long count = 0;
    if (f_contact && n) HIPCHK(hipMemcpyAsync(f_contact, ctx->d_rx_node, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (f_anchor && n) HIPCHK(hipMemcpyAsync(f_anchor, ctx->d_rx_node + 3 * n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&count, ctx->d_rx_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    I.n_contacts = count;
    if (info) *info = I;
    return ADMM_OK;
}

int admm_hip_get_contacts(admm_hip_ctx *ctx, double depth_min, admm_hip_contact *records, int64_t capacity, int64_t *count) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!(depth_min >= 0.0) || capacity < 0 || (capacity && !records)) return fail(ctx, ADMM_ERR_ARG, "get_contacts: depth_min must be >= 0 (got %g), capacity >= 0 and records given with it", depth_min);
    TRY(require_reactions(ctx, "get_contacts"));
    TRY(ensure_reaction_buffers(ctx));
    TRY(launch_contact_chain(ctx, depth_min, CHAIN_RECORDS));
    // (the count is not known before the synchronisation: the copy covers what the capacity could hold, the caller gets the filled part)
    static_assert(sizeof(admm_hip_contact) == sizeof(admm_dev::ContactRecord), "admm_hip_contact is the device's record");
    const size_t want = (size_t)std::min<int64_t>(capacity, ctx->n_nodes);
    std::vector<admm_hip_contact> tmp(want);
    long long c = 0;
    if (want) HIPCHK(hipMemcpyAsync(tmp.data(), ctx->d_rx_rec, sizeof(admm_hip_contact) * want, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&c, ctx->d_rx_count, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t k = (size_t)std::min<long long>(c, (long long)want);
    if (k) std::memcpy(records, tmp.data(), sizeof(admm_hip_contact) * k);
    if (count) *count = c;
    return ADMM_OK;
}

int admm_hip_contact_resultant(admm_hip_ctx *ctx, double depth_min, const double pivot[3], double out6[6], int64_t *count) {
    using namespace admm_dev;
    if (!ctx) return ADMM_ERR_ARG;
    if (!(depth_min >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "contact_resultant: depth_min must be >= 0, got %g", depth_min);
    TRY(require_reactions(ctx, "contact_resultant"));
    TRY(ensure_reaction_buffers(ctx));
    TRY(launch_contact_chain(ctx, depth_min, CHAIN_RECORDS));
    const EntryWork W = entry_work(ctx, false);      // one row: all contacts, in the records' order
    TRY(launch_row_sums(ctx, W, pivot));
    double h[6]; long long c = 0;
    HIPCHK(hipMemcpyAsync(h, W.out, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&c, ctx->d_rx_count, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (out6) for (int q = 0; q < 6; ++q) out6[q] = h[q];
    if (count) *count = c;
    return ADMM_OK;
}

// ---- contact attribution (attribution.hpp; include/admm_hip.h "contact attribution") ---------------------------------------------------
// The switch changes which kernel the collision batches launch (collision_plan.hpp: form 8), so it drops the captured graphs like a setter
// that changes the form (abi_setup.inc: push_shapes); the reports below read the record form 8 writes and change nothing a frame reads.
int admm_hip_enable_contact_attribution(admm_hip_ctx *ctx, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    const bool want = on != 0;
    if (!want) for (size_t mi = 0; mi < ctx->meshes.size(); ++mi) if (ctx->meshes[mi].reaction_share > 0.0)      // (abi_surface_reaction.inc)
        return fail(ctx, ADMM_ERR_STATE, "enable_contact_attribution: surface %d has a reaction share of %g, which needs every contact's owner entry: set it to 0 first", (int)mi, ctx->meshes[mi].reaction_share);
    if (!want && !ctx->rigid.empty())      // (abi_rigid.inc)
        return fail(ctx, ADMM_ERR_STATE, "enable_contact_attribution: entry %d is a rigid body, whose load needs every contact's owner entry", ctx->rigid[0].K.entry);
    if (want && ctx->finalized && ctx->device_id >= 0) { TRY(attribution_allocate(ctx)); TRY(attribution_fill(ctx)); }      // (before finalize: finalize does both)
    if (want != ctx->attribution) drop_iteration_graphs(ctx);
    ctx->attribution = want;
    return ADMM_OK;
}

static int require_attribution(admm_hip_ctx *ctx, const char *who) {
    TRY(require_reactions(ctx, who));
    if (!ctx->attribution) return fail(ctx, ADMM_ERR_STATE, "%s: contact attribution is off (admm_hip_enable_contact_attribution)", who);
    return ADMM_OK;
}

// the reports' buffers and, parallel to the gather's collision CSR, where every entry's element sits in the record; created by the first report
static int ensure_attribution_buffers(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    TRY(ensure_reaction_buffers(ctx));
    if (ctx->at_ready) return ADMM_OK;
    const int n = ctx->n_nodes, rows = ADMM_MAX_SHAPES + 1;
    const EntryWork W = entry_work(ctx, true);      // (the sizes alone: the pointers are being created)
    if (!ctx->d_at_rec) { OwnerRecord *r = nullptr; TRY(dalloc(ctx, &r, (size_t)std::max(n, 1))); ctx->d_at_rec = r; }
    if (!ctx->d_at_blk) TRY(dalloc(ctx, &ctx->d_at_blk, 2 * (size_t)rows * W.nblk));
    if (!ctx->d_at_tot) TRY(dalloc(ctx, &ctx->d_at_tot, (size_t)rows));
    if (!ctx->d_at_perm) TRY(dalloc(ctx, &ctx->d_at_perm, (size_t)std::max(n, 1)));
    if (!ctx->d_at_part) TRY(dalloc(ctx, &ctx->d_at_part, 6 * (size_t)W.n_part));
    if (!ctx->d_at_out) TRY(dalloc(ctx, &ctx->d_at_out, 6 * (size_t)rows));
    if (!ctx->d_at_csr) {
        std::vector<NodeCsrEntry> entries;      // (the order of ensure_reaction_buffers' collision entries: the two CSRs share ptr)
        for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_COLLISION)
            for (int el = 0; el < b.n_local; ++el) entries.push_back({b.idx[b.local[el]], b.at_off + el, 1});
        TRY(upload(ctx, &ctx->d_at_csr, build_node_csr(n, entries).off));
    }
    ctx->at_ready = true;
    return ADMM_OK;
}

int admm_hip_batch_contact_owner(admm_hip_ctx *ctx, int batch, int32_t *entry, double *normal) {
    if (!ctx) return ADMM_ERR_ARG;
    if (batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (b.kind != ADMM_KIND_COLLISION) return fail(ctx, ADMM_ERR_UNSUPPORTED, "batch_contact_owner: batch %d (kind %d) is not a collision batch", batch, b.kind);
    TRY(require_attribution(ctx, "batch_contact_owner"));
    HIPCHK(hipSetDevice(ctx->device_id));
    const int n = b.n_local;
    std::vector<double> t(3 * (size_t)std::max(n, 1), 0.0);
    if (n && entry) HIPCHK(hipMemcpyAsync(entry, ctx->d_at_owner + b.at_off, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (n && normal) for (int j = 0; j < 3; ++j)
        HIPCHK(hipMemcpyAsync(t.data() + (size_t)j * n, ctx->d_at_normal + (size_t)j * (size_t)ctx->at_total + b.at_off, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (normal) to_element_major(t, 3, n, normal);
    return ADMM_OK;
}

int admm_hip_get_contact_owners(admm_hip_ctx *ctx, double depth_min, admm_hip_contact_owner *records, int64_t capacity, int64_t *count) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!(depth_min >= 0.0) || capacity < 0 || (capacity && !records)) return fail(ctx, ADMM_ERR_ARG, "get_contact_owners: depth_min must be >= 0 (got %g), capacity >= 0 and records given with it", depth_min);
    TRY(require_attribution(ctx, "get_contact_owners"));
    TRY(ensure_attribution_buffers(ctx));
    TRY(launch_contact_chain(ctx, depth_min, CHAIN_OWNERS));
    static_assert(sizeof(admm_hip_contact_owner) == sizeof(admm_dev::OwnerRecord), "admm_hip_contact_owner is the device's record");
    const size_t want = (size_t)std::min<int64_t>(capacity, ctx->n_nodes);      // (as admm_hip_get_contacts: the count is not known before the synchronisation)
    std::vector<admm_hip_contact_owner> tmp(want);
    long long c = 0;
    if (want) HIPCHK(hipMemcpyAsync(tmp.data(), ctx->d_at_rec, sizeof(admm_hip_contact_owner) * want, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&c, ctx->d_rx_count, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t k = (size_t)std::min<long long>(c, (long long)want);
    if (k) std::memcpy(records, tmp.data(), sizeof(admm_hip_contact_owner) * k);
    if (count) *count = c;
    return ADMM_OK;
}

int admm_hip_entry_resultants(admm_hip_ctx *ctx, double depth_min, const double pivot[3], int n_entries, double *out, int64_t *count) {
    using namespace admm_dev;
    if (!ctx) return ADMM_ERR_ARG;
    if (!(depth_min >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "entry_resultants: depth_min must be >= 0, got %g", depth_min);
    if (n_entries != ctx->shapes.n || n_entries > ADMM_MAX_SHAPES) return fail(ctx, ADMM_ERR_ARG, "entry_resultants: %d entries given, the shape list has %d", n_entries, ctx->shapes.n);
    TRY(require_attribution(ctx, "entry_resultants"));
    TRY(ensure_attribution_buffers(ctx));
    TRY(launch_contact_chain(ctx, depth_min, CHAIN_RECORDS | CHAIN_OWNERS | CHAIN_SORTED));
    const EntryWork W = entry_work(ctx, true);
    TRY(launch_row_sums(ctx, W, pivot));
    const int rows = W.rows;
    std::vector<double> h(6 * (size_t)rows); std::vector<long long> c((size_t)rows);
    HIPCHK(hipMemcpyAsync(h.data(), W.out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(c.data(), W.totals, sizeof(long long) * c.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (out) std::copy(h.begin(), h.end(), out);
    if (count) for (int q = 0; q < rows; ++q) count[q] = c[q];
    return ADMM_OK;
}
