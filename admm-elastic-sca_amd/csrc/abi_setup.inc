// abi_setup.inc -- C ABI: context, nodes, batches, explicit forces, shapes, sharding, finalize (System::add_nodes / forces.push_back / initialize)
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)

// every entry's frame back to the identity about the origin
static void reset_frames(admm_hip_ctx *ctx) {
    for (int j = 0; j < ADMM_MAX_SHAPES; ++j) {
        for (int k = 0; k < 12; ++k) ctx->shapes.frame[j][k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        ctx->shapes.framed[j] = 0;
    }
}

int admm_hip_create(admm_hip_ctx **out, int device_id) {
    if (!out) return ADMM_ERR_ARG;
    *out = nullptr;
    admm_hip_ctx *ctx = new admm_hip_ctx();
    ctx->device_id = device_id;
    if (device_id >= 0) {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= device_id) {
            fprintf(stderr, "admm_hip: no HIP device %d (%s, %d devices) -- refusing to run without a GPU\n", device_id, hipGetErrorString(e), count);
            delete ctx;
            return ADMM_ERR_HIP;
        }
        if (hipSetDevice(device_id) != hipSuccess) { delete ctx; return ADMM_ERR_HIP; }
        if (hipStreamCreate(&ctx->stream) != hipSuccess) { delete ctx; return ADMM_ERR_HIP; }
        ctx->own_stream = true;
    }
    ctx->info.device_id = device_id; ctx->info.world = 1;
    reset_frames(ctx);
    const char *ls = getenv("ADMM_HIP_LEAF");
    if (ls && atoi(ls) > 0) ctx->leaf_size = atoi(ls);
    if (const char *g = getenv("ADMM_HIP_GRAPH")) { ctx->graph_enabled = atoi(g) != 0; ctx->graph_forced = ctx->graph_enabled; }
#if defined(ADMM_TET_PROFILE) || defined(ADMM_TET_TIMELINE) || defined(ADMM_SWEEP_PROFILE)
    ctx->graph_enabled = false;      // diagnostic builds: eager launches only (their per-launch symbol updates are not capturable)
#endif
    if (const char *g = getenv("ADMM_HIP_GRAPH_COMM")) ctx->graph_comm = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_BWD_NW")) { const int v = atoi(g); if (v == 4 || v == 8 || v == 16) ctx->knobs.bwd_nw = v; }
    if (const char *g = getenv("ADMM_HIP_FWD_SMALL_K")) ctx->knobs.fwd_small_k = atoi(g);
    if (const char *g = getenv("ADMM_HIP_BWD_SMALL_K")) ctx->knobs.bwd_small_k = atoi(g);
    if (const char *g = getenv("ADMM_HIP_TREE_SEARCH")) ctx->tree_search = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_STATE_DIRECT")) ctx->state_direct_max_nodes = atoi(g);      // systems up to that many nodes: upload_state / download_state without DMA (0: never)
    if (const char *g = getenv("ADMM_HIP_LOCAL_MULTI")) ctx->local_multi = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_TOP_BWD_ALL")) ctx->top_bwd_needed_only = atoi(g) == 0;
    if (const char *g = getenv("ADMM_HIP_ROOT_FUSE_K")) ctx->root_fuse_k = std::min(atoi(g), (int)admm_dev::ROOT_KCHUNK);
    if (const char *g = getenv("ADMM_HIP_FRAME_GRAPH")) ctx->frame_graph_on = atoi(g) != 0;      // 0: one graph launch per ADMM iteration instead of one per frame
    if (const char *g = getenv("ADMM_HIP_BWD_SMALL_NW")) { const int v = atoi(g); if (v == 2 || v == 4 || v == 8 || v == 16) ctx->knobs.bwd_small_nw = v; }
    if (const char *g = getenv("ADMM_HIP_XCD")) ctx->knobs.xcd_min_supernodes = atoi(g);
    if (const char *g = getenv("ADMM_HIP_TET_ORDER")) ctx->tet_order = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_TET_ORDER_MIN")) ctx->tet_order_min_blocks = atoi(g);
    if (const char *g = getenv("ADMM_HIP_FUSE_ANCHORS")) ctx->fuse_anchor_tail = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_FACTOR")) ctx->device_factor = std::string(g) != "host";
    if (const char *g = getenv("ADMM_HIP_BWD_CW2_MIN")) ctx->knobs.bwd_cw2_min_cols = atoi(g);
    if (const char *g = getenv("ADMM_HIP_BWD_CW2_MAX")) ctx->knobs.bwd_cw2_max_cols = atoi(g);
    if (const char *g = getenv("ADMM_HIP_PRERED")) ctx->tet_prered = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_STATE_ZEROCOPY")) ctx->state_zero_copy = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_TPB")) { const int v = atoi(g); if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) ctx->tet_tpb = v; }
    if (const char *g = getenv("ADMM_HIP_KEEP_Z")) ctx->keep_z_user = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_BWD_NW_MIN_COLS")) ctx->knobs.bwd_nw_min_cols = atoi(g);
    if (const char *g = getenv("ADMM_HIP_FWD_NW16_TILES")) ctx->knobs.fwd_nw16_max_tiles = atoi(g);
    if (const char *g = getenv("ADMM_HIP_FWD_NW4")) ctx->knobs.fwd_nw4_kmax = atoi(g);
    if (const char *g = getenv("ADMM_HIP_FWD_NW8")) ctx->knobs.fwd_nw8_kmax = atoi(g);
    if (const char *g = getenv("ADMM_HIP_DENSE_MAX")) ctx->dense_max = atoi(g);
    if (const char *g = getenv("ADMM_HIP_ROOT_INVERSE")) ctx->knobs.root_inverse = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_DIST_TOP")) ctx->dist_top_wanted = atoi(g) != 0 ? 1 : 0;
    if (const char *g = getenv("ADMM_HIP_DIST_TOP_MIN_NODES")) ctx->dist_top_min_nodes = atoi(g);
    if (const char *g = getenv("ADMM_HIP_SWEEP_FUSE")) ctx->knobs.sweep_fuse = atoi(g) != 0;
    if (const char *g = getenv("ADMM_HIP_SWEEP_FUSE_BWD")) ctx->knobs.sweep_fuse_bwd = atoi(g) != 0;
    *out = ctx;
    return ADMM_OK;
}

void admm_hip_destroy(admm_hip_ctx *ctx) {
    if (!ctx) return;
    if (ctx->device_id >= 0) {
        (void)hipSetDevice(ctx->device_id);
        (void)hipDeviceSynchronize();
        free_device(ctx);
        for (hipEvent_t e : ctx->evpool) (void)hipEventDestroy(e);
        for (hipEvent_t e : ctx->evpool_prev) (void)hipEventDestroy(e);
        comm_release(ctx);      // (comm.cpp: an owned RCCL communicator, the host-hook staging)
        for (double *h : {ctx->h_gen_dx, ctx->h_gen_u, ctx->h_gen_z, ctx->h_gen_q}) if (h) (void)hipHostFree(h);
        if (ctx->gen_ev) (void)hipEventDestroy(ctx->gen_ev);
        if (ctx->h_state) (void)hipHostFree(ctx->h_state);
        if (ctx->state_in_ev) (void)hipEventDestroy(ctx->state_in_ev);
        if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

const char *admm_hip_last_error(const admm_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int admm_hip_set_stream(admm_hip_ctx *ctx, void *s) {
    if (!ctx || ctx->device_id < 0) return ADMM_ERR_ARG;
    // the outgoing stream's work is finished first, a caller's stream too: nothing orders the next stream behind it (two non-blocking
    // streams, or a non-blocking and a blocking one, run side by side), and the frames queued there write what the next frame reads
    if (ctx->stream) { HIPCHK(hipSetDevice(ctx->device_id)); (void)hipStreamSynchronize(ctx->stream); }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->own_stream = false;
    ctx->stream = (hipStream_t)s;
    if (!s) { HIPCHK(hipStreamCreate(&ctx->stream)); ctx->own_stream = true; }
    return ADMM_OK;
}

int admm_hip_set_timestep(admm_hip_ctx *ctx, double dt) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "timestep cannot change after finalize (System.hpp:40)");
    ctx->dt = dt;
    return ADMM_OK;
}

int admm_hip_add_nodes(admm_hip_ctx *ctx, int n_nodes, const double *x, const double *m, int *total) {
    if (!ctx || n_nodes < 0 || (n_nodes && (!x || !m))) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "nodes cannot be added after finalize (System.hpp:60-62)");
    ctx->x.insert(ctx->x.end(), x, x + 3 * (size_t)n_nodes);
    ctx->m3.insert(ctx->m3.end(), m, m + 3 * (size_t)n_nodes);
    ctx->v.resize(ctx->x.size(), 0.0);
    ctx->n_nodes += n_nodes;
    if (total) *total = ctx->n_nodes;
    return ADMM_OK;
}

int admm_hip_add_batch(admm_hip_ctx *ctx, int kind, int n_elems, const int32_t *idx, const double *params, const double *targets, int *batch) {
    if (!ctx || n_elems < 0 || (n_elems && (!idx || !params))) return ADMM_ERR_ARG;
    if (kind < 0 || kind >= ADMM_KIND_COUNT) return fail(ctx, ADMM_ERR_UNSUPPORTED, "force kind %d has no accelerated kernel", kind);
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "forces cannot be added after finalize");
    Batch b; b.kind = kind; b.n_total = n_elems;
    b.idx.assign(idx, idx + (size_t)n_elems * ADMM_KIND_NODES[kind]);
    b.params.assign(params, params + (size_t)n_elems * ADMM_KIND_PARAMS[kind]);
    if (kind == ADMM_KIND_ANCHOR) {
        b.targets.assign((size_t)3 * n_elems, 0.0);
        b.active.assign(n_elems, 1);
        if (targets) {
            b.moving = true;
            std::copy(targets, targets + (size_t)3 * n_elems, b.targets.begin());
            for (int e = 0; e < n_elems; ++e) b.active[e] = params[2 * (size_t)e + 1] != 0.0;
        }
    }
    ctx->batches.push_back(std::move(b));
    if (batch) *batch = (int)ctx->batches.size() - 1;
    return ADMM_OK;
}

int admm_hip_add_generic_batch(admm_hip_ctx *ctx, int n_elems, const int32_t *elem_row_ptr, int64_t n_triplets, const int32_t *trip_row, const int32_t *trip_col,
                               const double *trip_val, const double *row_weight, int *batch) {
    if (!ctx || n_elems < 0 || n_triplets < 0 || !elem_row_ptr || (n_triplets && (!trip_row || !trip_col || !trip_val))) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "forces cannot be added after finalize");
    Batch b; b.kind = ADMM_KIND_GENERIC; b.n_total = n_elems;
    b.g_elem_row.assign(elem_row_ptr, elem_row_ptr + n_elems + 1);
    if (b.g_elem_row[0] != 0) return fail(ctx, ADMM_ERR_ARG, "generic batch: elem_row_ptr[0] must be 0");
    for (int e = 0; e < n_elems; ++e) if (b.g_elem_row[e + 1] < b.g_elem_row[e]) return fail(ctx, ADMM_ERR_ARG, "generic batch: elem_row_ptr must not decrease");
    const int64_t rows = b.g_elem_row[n_elems];
    if (rows && !row_weight) return ADMM_ERR_ARG;
    b.g_rows = rows; b.g_row0 = ctx->n_gen_rows;
    b.g_roww.assign(row_weight, row_weight + rows);
    // triplets -> CSR: ascending (row, column), duplicates summed in the order given (Eigen's setFromTriplets sums them too)
    std::vector<int64_t> ord(n_triplets);
    std::iota(ord.begin(), ord.end(), (int64_t)0);
    for (int64_t t = 0; t < n_triplets; ++t) if (trip_row[t] < 0 || trip_row[t] >= rows || trip_col[t] < 0) return fail(ctx, ADMM_ERR_ARG, "generic batch: triplet %lld (row %d, col %d) out of range (%lld rows)", (long long)t, trip_row[t], trip_col[t], (long long)rows);
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t c) { return trip_row[a] != trip_row[c] ? trip_row[a] < trip_row[c] : trip_col[a] < trip_col[c]; });
    b.g_rowptr.assign(rows + 1, 0);
    for (int64_t q = 0; q < n_triplets; ++q) {
        const int64_t t = ord[q];
        if (!b.g_col.empty() && q > 0 && trip_row[ord[q - 1]] == trip_row[t] && b.g_col.back() == trip_col[t]) { b.g_val.back() += trip_val[t]; continue; }
        b.g_col.push_back(trip_col[t]); b.g_val.push_back(trip_val[t]); b.g_rowptr[trip_row[t] + 1]++;
    }
    for (int64_t r = 0; r < rows; ++r) b.g_rowptr[r + 1] += b.g_rowptr[r];
    b.g_elem_node.assign(1, 0);
    for (int e = 0; e < n_elems; ++e) {
        std::vector<int32_t> nd;
        for (int64_t p = b.g_rowptr[b.g_elem_row[e]]; p < b.g_rowptr[b.g_elem_row[e + 1]]; ++p) nd.push_back(b.g_col[p] / 3);
        std::sort(nd.begin(), nd.end()); nd.erase(std::unique(nd.begin(), nd.end()), nd.end());
        b.g_nodes.insert(b.g_nodes.end(), nd.begin(), nd.end());
        b.g_elem_node.push_back((int64_t)b.g_nodes.size());
    }
    ctx->n_gen_rows += rows;
    ctx->batches.push_back(std::move(b));
    if (batch) *batch = (int)ctx->batches.size() - 1;
    return ADMM_OK;
}
int admm_hip_set_project_hook(admm_hip_ctx *ctx, admm_hip_project_fn fn, void *user) {
    if (!ctx) return ADMM_ERR_ARG;
    ctx->project_hook = fn; ctx->project_user = user;
    return ADMM_OK;
}

int admm_hip_add_explicit(admm_hip_ctx *ctx, int type, const double *dir, int n_idx, const int32_t *idx, int *which) {
    if (!ctx || !dir || n_idx < 0 || (n_idx && !idx)) return ADMM_ERR_ARG;
    if (type != ADMM_EXPLICIT_CONST && type != ADMM_EXPLICIT_WIND) return fail(ctx, ADMM_ERR_UNSUPPORTED, "explicit force type %d", type);
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "explicit forces cannot be added after finalize");
    Explicit E; E.type = type; E.n = n_idx;
    for (int j = 0; j < 3; ++j) E.dir[j] = dir[j];
    E.idx.assign(idx, idx + (size_t)n_idx * (type == ADMM_EXPLICIT_WIND ? 3 : 1));
    for (int32_t v : E.idx) if (v < 0) return fail(ctx, ADMM_ERR_ARG, "negative node id in explicit force");
    const bool simple = type == ADMM_EXPLICIT_CONST && n_idx == 0;
    if (simple && ctx->explicit_simple && ctx->grav.n < admm_dev::MAX_GRAV) { double *g = ctx->grav.g[ctx->grav.n++]; g[0] = dir[0]; g[1] = dir[1]; g[2] = dir[2]; }
    else ctx->explicit_simple = false;
    ctx->explicits.push_back(std::move(E));
    if (which) *which = (int)ctx->explicits.size() - 1;
    return ADMM_OK;
}
int admm_hip_add_gravity(admm_hip_ctx *ctx, double gx, double gy, double gz) {
    const double d[3] = {gx, gy, gz};
    return admm_hip_add_explicit(ctx, ADMM_EXPLICIT_CONST, d, 0, nullptr, nullptr);
}
int admm_hip_set_gravity(admm_hip_ctx *ctx, int which, double gx, double gy, double gz) {
    if (!ctx || which < 0 || which >= (int)ctx->explicits.size()) return ADMM_ERR_ARG;
    double *d = ctx->explicits[which].dir;
    d[0] = gx; d[1] = gy; d[2] = gz;
    if (ctx->explicit_simple) { double *g = ctx->grav.g[which]; g[0] = gx; g[1] = gy; g[2] = gz; }
    return ADMM_OK;
}
// What a list may not ask of a body surface, which sits where its nodes are and moves with them -- checked wherever the list or one of
// its per-entry arguments changes (for a surface already registered) and at finalize, rule after rule in this order, each over all
// entries; a rule whose argument is null (translations: false) is not checked:
//   translations   an entry that names one carries no translation
//   mu             ... and no friction coefficient: the body's own is admm_hip_set_body_surface_friction
//   motion         ... and no rigid motion [n_shapes][9]: the surface's motion is its nodes'
//   frames         ... and no frame [n_shapes][12] (the identity rotation passes whatever its pivot)
static int check_body_entries(admm_hip_ctx *ctx, int n_shapes, const int32_t *types, const double *params, bool translations, const double *mu, const double *motion,
                              const double *frames) {
    int body[ADMM_MAX_SHAPES], nb = 0;      // the entries that name a body surface, and its id
    for (int j = 0; j < n_shapes; ++j) { const admm_hip_ctx::CollisionMesh *m = entry_mesh(ctx, types, params, j); if (m && m->body()) body[nb++] = j; }
    auto id = [&](int j) { return (int)params[4 * (size_t)j + 3]; };
    if (translations) for (int q = 0; q < nb; ++q) {
        const int j = body[q]; const double *p = params + 4 * (size_t)j;
        if (p[0] != 0.0 || p[1] != 0.0 || p[2] != 0.0)
            return fail(ctx, ADMM_ERR_ARG, "collision shape %d: mesh %d is a body surface, which follows its nodes: its translation must be 0 (have %g, %g, %g)", j, id(j), p[0], p[1], p[2]);
    }
    if (mu) for (int q = 0; q < nb; ++q) {
        const int j = body[q];
        if (mu[j] != 0.0) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: mesh %d is a body surface, which moves with its nodes: its friction coefficient must be 0 (have %g)", j, id(j), mu[j]);
    }
    if (motion) for (int q = 0; q < nb; ++q) {
        const int j = body[q];
        for (int k = 0; k < 9; ++k)
            if (motion[9 * (size_t)j + k] != 0.0)
                return fail(ctx, ADMM_ERR_ARG, "collision shape %d: mesh %d is a body surface, which moves with its nodes: its rigid motion must be 0 (component %d is %g)", j, id(j), k, motion[9 * (size_t)j + k]);
    }
    if (frames) for (int q = 0; q < nb; ++q) {
        const int j = body[q];
        if (!admm_frame::identity(frames + 12 * (size_t)j))
            return fail(ctx, ADMM_ERR_ARG, "collision shape %d: mesh %d is a body surface, which follows its nodes: its frame must be the identity", j, id(j));
    }
    return ADMM_OK;
}
// side memory: a node has one side per mesh, so a list names a mesh with memory in one entry at most
static int check_side_entries(admm_hip_ctx *ctx, int n_shapes, const int32_t *types, const double *params) {
    for (int j = 0; j < n_shapes; ++j) {
        const admm_hip_ctx::CollisionMesh *m = entry_mesh(ctx, types, params, j);
        if (!m || !(m->side_reach > 0.0)) continue;
        for (int k = 0; k < j; ++k)
            if (entry_mesh(ctx, types, params, k) == m)
                return fail(ctx, ADMM_ERR_ARG, "collision shapes %d and %d both name mesh %d, which has side memory: a node has one side per mesh", k, j, (int)params[4 * (size_t)j + 3]);
    }
    return ADMM_OK;
}
// a setter changed the shape table: once finalized it goes to the device again (between frames; the values change under a captured graph
// like shape parameters) -- with_motion: and the mesh motion table with it -- and a change of the collision batches' kernels (form_before:
// collision_form before the change) drops the captured graphs
static int push_shapes(admm_hip_ctx *ctx, int form_before, bool with_motion = false) {
    if (!ctx->finalized || ctx->device_id < 0) return ADMM_OK;
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipMemcpyAsync(ctx->d_shapes, &ctx->shapes, sizeof(admm_dev::ShapeTable), hipMemcpyHostToDevice, ctx->stream));
    const std::vector<admm_mesh::MeshMotion> mo = with_motion ? mesh_motion_table(ctx) : std::vector<admm_mesh::MeshMotion>();
    if (!mo.empty()) HIPCHK(hipMemcpyAsync(ctx->d_mesh_motion, mo.data(), sizeof(admm_mesh::MeshMotion) * mo.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (form_before != collision_form(ctx).form) drop_iteration_graphs(ctx);
    return ADMM_OK;
}
int admm_hip_set_collision_shapes(admm_hip_ctx *ctx, int n_shapes, const int32_t *types, const double *params) {
    if (!ctx || n_shapes < 0 || (n_shapes && (!types || !params))) return ADMM_ERR_ARG;
    if (n_shapes > ADMM_MAX_SHAPES) return fail(ctx, ADMM_ERR_UNSUPPORTED, "at most %d collision shapes", ADMM_MAX_SHAPES);
    for (int j = 0; j < n_shapes; ++j) {      // (checked before the table changes: a refused list leaves the last good one in place)
        if (types[j] < ADMM_SHAPE_FLOOR || types[j] > ADMM_SHAPE_BOX) return fail(ctx, ADMM_ERR_UNSUPPORTED, "collision shape type %d", types[j]);
        if (types[j] == ADMM_SHAPE_MESH) {
            const double id = params[4 * (size_t)j + 3];
            if (!(id >= 0.0 && id < (double)ctx->meshes.size() && id == (double)(int)id))
                return fail(ctx, ADMM_ERR_ARG, "collision shape %d: mesh_id %g is not a registered mesh (have %d)", j, id, (int)ctx->meshes.size());
        }
        if (types[j] == ADMM_SHAPE_BOX)
            for (int k = 0; k < 3; ++k) {
                const double h = params[4 * (size_t)j + k];
                if (!(h > 0.0 && std::isfinite(h))) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: the box's half extent %d is %g: it must be positive and finite", j, k, h);
            }
    }
    TRY(check_body_entries(ctx, n_shapes, types, params, true, nullptr, nullptr, nullptr));
    TRY(check_side_entries(ctx, n_shapes, types, params));
    // rigid bodies (abi_rigid.inc) are entries of THIS list: its length stands while one exists, a body's entry keeps its type, and its
    // params are the body's own (the device rewrites them at every step), not the caller's
    if (!ctx->rigid.empty() && n_shapes != ctx->shapes.n)
        return fail(ctx, ADMM_ERR_STATE, "collision shapes: a list of %d entries while entry %d of the current %d is a rigid body: the list keeps its length while bodies exist", n_shapes,
                    ctx->rigid[0].K.entry, ctx->shapes.n);
    for (const admm_hip_ctx::RigidBodyHost &B : ctx->rigid)
        if (types[B.K.entry] != B.K.type)
            return fail(ctx, ADMM_ERR_ARG, "collision shape %d is a rigid body of type %d: its type cannot change to %d", B.K.entry, B.K.type, types[B.K.entry]);
    // (a list of the same length keeps its coefficients, motions and frames: one that now names a body surface where one of them is set is
    //  refused here -- a coefficient once finalized, by finalize before)
    if (n_shapes == ctx->shapes.n)
        TRY(check_body_entries(ctx, n_shapes, types, params, false, ctx->finalized ? ctx->shapes.mu : nullptr, &ctx->shapes.motion[0][0], &ctx->shapes.frame[0][0]));
    const int form = collision_form(ctx).form;
    if (n_shapes != ctx->shapes.n) {      // a list of another length: its coefficients and motions start at 0, its frames at the identity (the same length keeps them)
        for (double &m : ctx->shapes.mu) m = 0.0;
        for (auto &m : ctx->shapes.motion) for (double &c : m) c = 0.0;
        reset_frames(ctx);
    }
    ctx->shapes.n = n_shapes;
    for (int j = 0; j < n_shapes; ++j) {
        ctx->shapes.type[j] = types[j];
        bool rigid = false;
        for (const admm_hip_ctx::RigidBodyHost &B : ctx->rigid) rigid |= B.K.entry == j;
        if (!rigid) for (int q = 0; q < 4; ++q) ctx->shapes.par[j][q] = params[4 * (size_t)j + q];
    }
    return push_shapes(ctx, form);
}

// extension, no reference counterpart (include/admm_hip.h): one Coulomb coefficient per entry of the current shape list.  The values live in
// d_shapes and change under a captured graph like shape parameters; only a change between "all zero" and "some positive" changes which
// kernels the collision batches launch, and drops the captured graphs.
int admm_hip_set_collision_friction(admm_hip_ctx *ctx, int n_shapes, const double *mu) {
    if (!ctx) return ADMM_ERR_ARG;
    if (n_shapes != ctx->shapes.n) return fail(ctx, ADMM_ERR_ARG, "collision friction: %d coefficients given, the shape list has %d entries", n_shapes, ctx->shapes.n);
    if (n_shapes && !mu) return fail(ctx, ADMM_ERR_ARG, "collision friction: no coefficients");
    for (int j = 0; j < n_shapes; ++j)
        if (!(mu[j] >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: friction coefficient %g is negative or not a number", j, mu[j]);
    TRY(check_body_entries(ctx, n_shapes, ctx->shapes.type, &ctx->shapes.par[0][0], false, mu, nullptr, nullptr));
    const int form = collision_form(ctx).form;
    for (int j = 0; j < n_shapes; ++j) ctx->shapes.mu[j] = mu[j];
    return push_shapes(ctx, form);
}

// extension, no reference counterpart (include/admm_hip.h): the rigid frame of every entry of the current list (NULL: the identity)
int admm_hip_set_collision_frames(admm_hip_ctx *ctx, int n_shapes, const double *frames) {
    if (!ctx) return ADMM_ERR_ARG;
    if (n_shapes != ctx->shapes.n) return fail(ctx, ADMM_ERR_ARG, "collision frames: %d frames given, the shape list has %d entries", n_shapes, ctx->shapes.n);
    if (frames) {
        for (int j = 0; j < n_shapes; ++j) {
            int which = 0; double by = 0.0;
            const int bad = admm_frame::check(frames + 12 * (size_t)j, &which, &by);
            if (bad == 1) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: frame component %d is not finite (%g)", j, which, by);
            if (bad == 2 && which < 9) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: its frame's R is not a rotation: element (%d, %d) of R^T R - I is %g, beyond 1e-12", j, which / 3, which % 3, by);
            if (bad == 2) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: its frame's R is not a rotation: det R - 1 is %g, beyond 1e-12", j, by);
        }
        TRY(check_body_entries(ctx, n_shapes, ctx->shapes.type, &ctx->shapes.par[0][0], false, nullptr, nullptr, frames));
    }
    const int form = collision_form(ctx).form;
    if (!frames) reset_frames(ctx);
    else for (int j = 0; j < n_shapes; ++j) {
        for (int k = 0; k < 12; ++k) ctx->shapes.frame[j][k] = frames[12 * (size_t)j + k];
        ctx->shapes.framed[j] = admm_frame::identity(ctx->shapes.frame[j]) ? 0 : 1;
    }
    return push_shapes(ctx, form);
}

// extension, no reference counterpart (include/admm_hip.h): the rigid motion of every entry of the current list
int admm_hip_set_collision_motion(admm_hip_ctx *ctx, int n_shapes, const double *motion) {
    if (!ctx) return ADMM_ERR_ARG;
    if (n_shapes != ctx->shapes.n) return fail(ctx, ADMM_ERR_ARG, "collision motion: %d motions given, the shape list has %d entries", n_shapes, ctx->shapes.n);
    if (n_shapes && !motion) return fail(ctx, ADMM_ERR_ARG, "collision motion: no motions");
    for (int j = 0; j < n_shapes; ++j)
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(motion[9 * (size_t)j + k])) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: motion component %d is not finite (%g)", j, k, motion[9 * (size_t)j + k]);
    TRY(check_body_entries(ctx, n_shapes, ctx->shapes.type, &ctx->shapes.par[0][0], false, nullptr, motion, nullptr));
    const int form = collision_form(ctx).form;
    for (int j = 0; j < n_shapes; ++j) for (int k = 0; k < 9; ++k) ctx->shapes.motion[j][k] = motion[9 * (size_t)j + k];
    return push_shapes(ctx, form, true);
}

// ... the velocity of every vertex of a registered obstacle mesh (vel NULL: none again)
int admm_hip_set_collision_mesh_velocity(admm_hip_ctx *ctx, int mesh_id, int nv, const double *vel) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "collision mesh velocities are set after finalize");
    admm_hip_ctx::CollisionMesh *mv = mesh_by_id(ctx, mesh_id);
    if (!mv) return ADMM_ERR_ARG;
    if (mv->body())
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is a body surface, which moves with its nodes: it takes no velocities from the caller", mesh_id);
    const admm_hip_mesh &M = mv->mesh;
    if (vel && nv != M.nv) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: %d vertex velocities given, the mesh has %d vertices", mesh_id, nv, M.nv);
    if (vel) for (int v = 0; v < nv; ++v)
        if (!admm_mesh::finite3(vel + 3 * (size_t)v)) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: the velocity of vertex %d is not finite", mesh_id, v);
    const int form = collision_form(ctx).form;
    if (vel && ctx->device_id >= 0) {
        HIPCHK(hipSetDevice(ctx->device_id));
        if (!mv->d_vel) { TRY(dalloc(ctx, &mv->d_vel, 3 * (size_t)nv)); drop_iteration_graphs(ctx); }      // (allocated here, never by admm_hip_step)
        HIPCHK(hipMemcpyAsync(mv->d_vel, vel, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice, ctx->stream));
    }
    if (vel) mv->vel.assign(vel, vel + 3 * (size_t)nv); else mv->vel.clear();
    mv->has_vel = vel != nullptr;
    return push_shapes(ctx, form, true);
}

// ... the coefficient of a body surface: of the body, for every entry that names the surface
int admm_hip_set_body_surface_friction(admm_hip_ctx *ctx, int mesh_id, double mu) {
    if (!ctx) return ADMM_ERR_ARG;
    if (mesh_id < 0 || mesh_id >= (int)ctx->meshes.size() || !ctx->meshes[mesh_id].body())
        return fail(ctx, ADMM_ERR_ARG, "mesh_id %d is not a body surface", mesh_id);
    if (!(mu >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "body surface %d: friction coefficient %g is negative or not a number", mesh_id, mu);
    const int form = collision_form(ctx).form;
    ctx->meshes[mesh_id].body_mu = mu;
    return push_shapes(ctx, form, true);
}

// a mesh becomes a registered one: the context's record of it, everything but the mesh itself at its default (an obstacle without an owner)
static admm_hip_ctx::CollisionMesh &register_mesh(admm_hip_ctx *ctx, const admm_hip_mesh &mesh, int *mesh_id) {
    ctx->meshes.emplace_back();
    ctx->meshes.back().mesh = mesh;
    if (mesh_id) *mesh_id = (int)ctx->meshes.size() - 1;
    return ctx->meshes.back();
}

// extension, no reference counterpart (include/admm_hip.h): the context keeps its own copy, uploaded at finalize
int admm_hip_add_collision_mesh(admm_hip_ctx *ctx, const admm_hip_mesh *mesh, int *mesh_id) {
    if (!ctx || !mesh || mesh->nodes.empty()) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "collision meshes must be registered before finalize");
    register_mesh(ctx, *mesh, mesh_id);
    return ADMM_OK;
}

// owner ranges of two meshes may be equal or disjoint (one body tag per node)
static int check_owner_range(admm_hip_ctx *ctx, int mesh_id, int first, int count) {
    if (first < 0 || count < 1 || first > ctx->n_nodes - count)
        return fail(ctx, ADMM_ERR_ARG, "node range [%d, %d) is not inside the %d nodes added so far", first, first + count, ctx->n_nodes);
    for (size_t i = 0; i < ctx->meshes.size(); ++i) {
        const admm_hip_ctx::CollisionMesh &R = ctx->meshes[i];
        if ((int)i == mesh_id || !R.own_count || (R.own_first == first && R.own_count == count)) continue;
        if (first < R.own_first + R.own_count && R.own_first < first + count)
            return fail(ctx, ADMM_ERR_ARG, "node range [%d, %d) overlaps the owner range [%d, %d) of mesh %d without being equal to it", first, first + count,
                        R.own_first, R.own_first + R.own_count, (int)i);
    }
    return ADMM_OK;
}

// extension, no reference counterpart (include/admm_hip.h): a closed surface of simulated nodes, rebuilt on the device from the frame-start
// x at every step (launch.inc: update_bodies); owned by its node range.  half_thickness > 0: an open one (admm_hip_add_sheet_surface)
static int add_node_surface(admm_hip_ctx *ctx, int node_first, int node_count, int n_tris, const int32_t *tris, double half_thickness, int *mesh_id) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "body surfaces must be registered before finalize");
    if (n_tris < 1 || !tris) return fail(ctx, ADMM_ERR_ARG, "body surface: no triangles");
    TRY(check_owner_range(ctx, -1, node_first, node_count));
    std::vector<int> nodes(tris, tris + 3 * (size_t)n_tris);
    for (size_t i = 0; i < nodes.size(); ++i)
        if (nodes[i] < node_first || nodes[i] >= node_first + node_count)
            return fail(ctx, ADMM_ERR_ARG, "body surface: triangle %d names node %d outside [%d, %d)", (int)(i / 3), nodes[i], node_first, node_first + node_count);
    std::sort(nodes.begin(), nodes.end());
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    std::vector<int> local((size_t)node_count, -1);
    std::vector<double> verts(3 * nodes.size());
    for (size_t k = 0; k < nodes.size(); ++k) {
        local[nodes[k] - node_first] = (int)k;
        for (int j = 0; j < 3; ++j) verts[3 * k + j] = ctx->x[3 * (size_t)nodes[k] + j];
    }
    std::vector<int32_t> lt(3 * (size_t)n_tris);
    for (size_t i = 0; i < lt.size(); ++i) lt[i] = local[tris[i] - node_first];
    admm_hip_mesh *M = nullptr;
    char msg[512];
    const int rc = half_thickness > 0.0 ? admm_hip_mesh_create_open(&M, (int)nodes.size(), verts.data(), n_tris, lt.data(), half_thickness, msg, (int)sizeof msg)
                                        : admm_hip_mesh_create(&M, (int)nodes.size(), verts.data(), n_tris, lt.data(), msg, (int)sizeof msg);
    if (rc) return fail(ctx, rc, "body surface: %s", msg);
    admm_hip_ctx::CollisionMesh &R = register_mesh(ctx, *M, mesh_id);
    admm_hip_mesh_destroy(M);
    R.own_first = node_first; R.own_count = node_count; R.body_nodes = std::move(nodes);
    if (!R.open()) R.rest = verts;      // a closed body surface keeps its rest shape (admm_hip_set_body_self_collision)
    return ADMM_OK;
}

int admm_hip_add_body_surface(admm_hip_ctx *ctx, int node_first, int node_count, int n_tris, const int32_t *tris, int *mesh_id) {
    return add_node_surface(ctx, node_first, node_count, n_tris, tris, 0.0, mesh_id);
}
// ... an open one, such as a cloth: a thick shell that follows its nodes
int admm_hip_add_sheet_surface(admm_hip_ctx *ctx, int node_first, int node_count, int n_tris, const int32_t *tris, double half_thickness, int *mesh_id) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!(half_thickness > 0.0 && std::isfinite(half_thickness))) return fail(ctx, ADMM_ERR_ARG, "sheet surface: half thickness %g: it must be positive and finite", half_thickness);
    return add_node_surface(ctx, node_first, node_count, n_tris, tris, half_thickness, mesh_id);
}

// extension, no reference counterpart (include/admm_hip.h): a sheet surface whose own nodes meet it outside their 1-ring instead of
// skipping it (project_collision_self_kernel); before finalize, which checks the rest pose against the half thickness
int admm_hip_set_sheet_self_collision(admm_hip_ctx *ctx, int mesh_id, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "sheet self-collision must be set before finalize");
    admm_hip_ctx::CollisionMesh *R = mesh_by_id(ctx, mesh_id);
    if (!R) return ADMM_ERR_ARG;
    if (!R->body())
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is an obstacle mesh, not a sheet surface: it has no nodes to collide with itself", mesh_id);
    if (!R->open())
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is a closed body surface, not a sheet surface: self-collision of a closed surface is not supported", mesh_id);
    R->self_collision = on != 0;
    return ADMM_OK;
}

// extension, no reference counterpart (include/admm_hip.h): a closed body surface whose surface nodes meet it outside what is near them in
// the rest shape (project_collision_bodyself_kernel, mesh_query.hpp); before finalize, which checks the finalize positions against the rule
int admm_hip_set_body_self_collision(admm_hip_ctx *ctx, int mesh_id, double r, double reach, double rest_radius) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "body self-collision must be set before finalize");
    admm_hip_ctx::CollisionMesh *Rp = mesh_by_id(ctx, mesh_id);
    if (!Rp) return ADMM_ERR_ARG;
    admm_hip_ctx::CollisionMesh &R = *Rp;
    if (!R.body())
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is an obstacle mesh, not a body surface: it has no nodes to collide with itself", mesh_id);
    if (R.open())
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is a sheet surface, not a closed body surface: use admm_hip_set_sheet_self_collision", mesh_id);
    if (!std::isfinite(r) || !std::isfinite(reach) || !std::isfinite(rest_radius))
        return fail(ctx, ADMM_ERR_ARG, "body surface %d: self-collision lengths r %g, reach %g, rest radius %g: a value is not finite", mesh_id, r, reach, rest_radius);
    if (r == 0.0) { R.body_self[0] = R.body_self[1] = R.body_self[2] = 0.0; return ADMM_OK; }
    if (!(r > 0.0)) return fail(ctx, ADMM_ERR_ARG, "body surface %d: half gap %g is negative", mesh_id, r);
    if (!(reach >= r)) return fail(ctx, ADMM_ERR_ARG, "body surface %d: reach %g is below the half gap %g", mesh_id, reach, r);
    if (!(rest_radius >= reach)) return fail(ctx, ADMM_ERR_ARG, "body surface %d: rest radius %g is below the reach %g", mesh_id, rest_radius, reach);
    R.body_self[0] = r; R.body_self[1] = reach; R.body_self[2] = rest_radius;
    return ADMM_OK;
}

// finalize: a body surface that collides with itself must be left alone by the rule where it stands (the positions finalize sees), or
// its nodes would be pushed from the first frame; and a node takes its vertex id from one self-colliding surface only, sheet or body
static int check_body_self_collision(admm_hip_ctx *ctx) {
    for (size_t i = 0; i < ctx->meshes.size(); ++i) {
        const admm_hip_ctx::CollisionMesh &R = ctx->meshes[i];
        if (!(R.body_self[0] > 0.0)) continue;
        for (size_t k = 0; k < ctx->meshes.size(); ++k) {      // (owner ranges overlap only when they are equal)
            const admm_hip_ctx::CollisionMesh &Q = ctx->meshes[k];
            if (k == i || Q.own_first != R.own_first || Q.own_count != R.own_count) continue;
            if (Q.self_collision || (k < i && Q.body_self[0] > 0.0))
                return fail(ctx, ADMM_ERR_ARG, "surfaces %d and %d both collide with themselves and share the node range [%d, %d): a node takes its vertex id from one such surface",
                            (int)std::min(i, k), (int)std::max(i, k), R.own_first, R.own_first + R.own_count);
        }
        admm_hip_mesh cur = R.mesh;
        std::vector<double> verts(3 * R.body_nodes.size());
        for (size_t k = 0; k < R.body_nodes.size(); ++k) for (int j = 0; j < 3; ++j) verts[3 * k + j] = ctx->x[3 * (size_t)R.body_nodes[k] + j];
        char msg[512];
        if (const int rc = admm_mesh::mesh_set_vertices(cur, cur.nv, verts.data(), msg, (int)sizeof msg)) return fail(ctx, rc, "body surface %d: %s", (int)i, msg);
        int v = -1, t = -1; double d = 0.0;
        if (admm_mesh::body_rest_violation(cur, R.rest.data(), R.body_self[0], R.body_self[1], R.body_self[2], &v, &t, &d)) {
            const int *c = cur.cid.data() + 3 * (size_t)t;
            return fail(ctx, ADMM_ERR_ARG, "body surface %d: vertex %d (node %d) lies at distance %g from triangle %d (%d, %d, %d), which is not near it in the rest shape (rest radius %g): "
                        "the rule (half gap %g, reach %g) would move it, the body would collide with itself where it stands", (int)i, v, R.body_nodes[v], d, t, c[0], c[1], c[2],
                        R.body_self[2], R.body_self[0], R.body_self[1]);
        }
    }
    return ADMM_OK;
}

// finalize: every sheet that collides with itself must be clear of itself where it stands -- no vertex nearer than the half thickness to
// a triangle it is not a corner of, or every node would be pushed by its own neighbourhood from the first frame -- and a node takes its
// vertex id from one such sheet only
static int check_sheet_self_collision(admm_hip_ctx *ctx) {
    for (size_t i = 0; i < ctx->meshes.size(); ++i) {
        const admm_hip_ctx::CollisionMesh &R = ctx->meshes[i];
        if (!R.self_collision) continue;
        for (size_t k = 0; k < i; ++k)      // (owner ranges overlap only when they are equal)
            if (ctx->meshes[k].self_collision && ctx->meshes[k].own_first == R.own_first && ctx->meshes[k].own_count == R.own_count)
                return fail(ctx, ADMM_ERR_ARG, "sheet surfaces %d and %d both collide with themselves and share the node range [%d, %d): a node takes its vertex id from one such sheet",
                            (int)k, (int)i, R.own_first, R.own_first + R.own_count);
        int v = -1, t = -1; double d = 0.0;
        if (admm_mesh::sheet_rest_violation(R.mesh, &v, &t, &d)) {
            const int *c = R.mesh.cid.data() + 3 * (size_t)t;
            return fail(ctx, ADMM_ERR_ARG, "sheet surface %d: vertex %d (node %d) lies at distance %g from triangle %d (%d, %d, %d), which it is not a corner of: nearer than the half "
                        "thickness %g, the sheet would collide with itself at rest", (int)i, v, R.body_nodes[v], d, t, c[0], c[1], c[2], R.mesh.thickness);
        }
    }
    return ADMM_OK;
}

// the half thickness of a registered open mesh, between frames: one entry of the device table project_collision_shell_kernel reads
// (no kernel changes, captured graphs stay)
int admm_hip_set_collision_mesh_thickness(admm_hip_ctx *ctx, int mesh_id, double half_thickness) {
    if (!ctx) return ADMM_ERR_ARG;
    admm_hip_ctx::CollisionMesh *m = mesh_by_id(ctx, mesh_id);
    if (!m) return ADMM_ERR_ARG;
    if (!m->open()) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is a closed mesh: it has no thickness", mesh_id);
    if (!(half_thickness > 0.0 && std::isfinite(half_thickness)))
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: half thickness %g: it must be positive and finite", mesh_id, half_thickness);
    if (m->side_reach > 0.0 && half_thickness > m->side_reach)
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: half thickness %g exceeds the reach %g of its side memory", mesh_id, half_thickness, m->side_reach);
    m->mesh.thickness = half_thickness;
    if (ctx->finalized && ctx->device_id >= 0) {
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipMemcpyAsync(ctx->d_mesh_thick + mesh_id, &m->mesh.thickness, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return ADMM_OK;
}

// extension, no reference counterpart (include/admm_hip.h): side memory for an open mesh (mesh_query.hpp); before finalize, which
// allocates one row of sides per such mesh
int admm_hip_set_collision_mesh_side_memory(admm_hip_ctx *ctx, int mesh_id, double reach) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "side memory must be set before finalize");
    admm_hip_ctx::CollisionMesh *m = mesh_by_id(ctx, mesh_id);
    if (!m) return ADMM_ERR_ARG;
    const double r = m->mesh.thickness;
    if (!(r > 0.0)) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is a closed mesh: it has an inside and needs no side memory", mesh_id);
    if (!std::isfinite(reach)) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: reach %g is not finite", mesh_id, reach);
    if (reach != 0.0 && !(reach >= r)) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: reach %g is below its half thickness %g", mesh_id, reach, r);
    if (reach != 0.0) {      // (the current list may already name it twice)
        const double before = m->side_reach;
        m->side_reach = reach;
        const int rc = check_side_entries(ctx, ctx->shapes.n, ctx->shapes.type, &ctx->shapes.par[0][0]);
        if (rc) { m->side_reach = before; return rc; }
    }
    m->side_reach = reach;
    return ADMM_OK;
}

int admm_hip_set_collision_mesh_owner(admm_hip_ctx *ctx, int mesh_id, int node_first, int node_count) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "mesh owners must be set before finalize");
    admm_hip_ctx::CollisionMesh *Rp = mesh_by_id(ctx, mesh_id);
    if (!Rp) return ADMM_ERR_ARG;
    admm_hip_ctx::CollisionMesh &R = *Rp;
    if (node_count == 0) { R.own_first = R.own_count = 0; return ADMM_OK; }
    TRY(check_owner_range(ctx, mesh_id, node_first, node_count));
    R.own_first = node_first; R.own_count = node_count;
    return ADMM_OK;
}

int admm_hip_get_body_surface_status(admm_hip_ctx *ctx, int mesh_id, int64_t *updated, int64_t *refused, int *last_bad_tri) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "body surface status before finalize");
    if (mesh_id < 0 || mesh_id >= (int)ctx->meshes.size() || !ctx->meshes[mesh_id].body())
        return fail(ctx, ADMM_ERR_ARG, "mesh_id %d is not a body surface", mesh_id);
    admm_mesh::BodyStatus st{0, 0, -1, 0};
    if (ctx->device_id >= 0) {
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipMemcpyAsync(&st, ctx->meshes[mesh_id].upd.status, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (updated) *updated = st.updated;
    if (refused) *refused = st.refused;
    if (last_bad_tri) *last_bad_tri = st.last_bad_tri;
    return ADMM_OK;
}

// a standalone copy of a context's registered mesh as registered (and as updated on the host: before finalize, host-only contexts)
int admm_hip_collision_mesh_copy(admm_hip_ctx *ctx, int mesh_id, admm_hip_mesh **out) {
    if (!ctx || !out) return ADMM_ERR_ARG;
    *out = nullptr;
    const admm_hip_ctx::CollisionMesh *m = mesh_by_id(ctx, mesh_id);
    if (!m) return ADMM_ERR_ARG;
    *out = new (std::nothrow) admm_hip_mesh(m->mesh);
    return *out ? ADMM_OK : fail(ctx, ADMM_ERR_ARG, "out of memory");
}

// before finalize (or in a host-only context) the context's copy takes admm_hip_mesh_set_vertices; after it the device arrays are
// rewritten in place (launch.inc: update_mesh_device)
int admm_hip_update_collision_mesh(admm_hip_ctx *ctx, int mesh_id, int nv, const double *verts) {
    if (!ctx) return ADMM_ERR_ARG;
    admm_hip_ctx::CollisionMesh *m = mesh_by_id(ctx, mesh_id);
    if (!m) return ADMM_ERR_ARG;
    if (m->body())
        return fail(ctx, ADMM_ERR_ARG, "collision mesh %d is a body surface, which follows its nodes: it takes no vertices from the caller", mesh_id);
    admm_hip_mesh &M = m->mesh;
    if (!ctx->finalized || ctx->device_id < 0) {
        char msg[512];
        const int rc = admm_mesh::mesh_set_vertices(M, nv, verts, msg, (int)sizeof msg);
        return rc ? fail(ctx, rc, "collision mesh %d: %s", mesh_id, msg) : ADMM_OK;
    }
    if (nv != M.nv || !verts) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: %d vertices given, the mesh has %d", mesh_id, nv, M.nv);
    HIPCHK(hipSetDevice(ctx->device_id));
    return update_mesh_device(ctx, mesh_id, verts);
}

int admm_hip_set_shard(admm_hip_ctx *ctx, int rank, int world) {
    if (!ctx || world < 1 || rank < 0 || rank >= world) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "shard must be set before finalize");
    if (world > 1) for (const admm_hip_ctx::CollisionMesh &m : ctx->meshes) if (m.reaction_share > 0.0)      // (abi_surface_reaction.inc)
        return fail(ctx, ADMM_ERR_UNSUPPORTED, "set_shard: a surface reaction share is set, which is not available in a sharded context (world = %d)", world);
    if (world > 1 && !ctx->rigid.empty())      // (abi_rigid.inc)
        return fail(ctx, ADMM_ERR_UNSUPPORTED, "set_shard: entry %d is a rigid body, which is not available in a sharded context (world = %d)", ctx->rigid[0].K.entry, world);
    ctx->rank = rank; ctx->world = world;
    return ADMM_OK;
}
int admm_hip_set_shard_mode(admm_hip_ctx *ctx, int mode) {
    if (!ctx || (mode != ADMM_SHARD_CONTIGUOUS && mode != ADMM_SHARD_SUBTREE)) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "shard mode must be set before finalize");
    ctx->shard_mode = mode;
    return ADMM_OK;
}
int admm_hip_set_factor_local(admm_hip_ctx *ctx, int on) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "factor_local must be set before finalize");
    ctx->factor_local = on != 0;
    return ADMM_OK;
}
int admm_hip_local_elements(admm_hip_ctx *ctx, int batch, int32_t *ids, int capacity, int *n_local) {
    if (!ctx || !ctx->finalized || batch < 0 || batch >= (int)ctx->batches.size()) return ADMM_ERR_ARG;
    const Batch &b = ctx->batches[batch];
    if (n_local) *n_local = b.n_local;
    if (ids) { if (capacity < b.n_local) return ADMM_ERR_ARG; std::copy(b.local.begin(), b.local.end(), ids); }
    return ADMM_OK;
}
int admm_hip_debug_node_owner(admm_hip_ctx *ctx, int32_t *owner) {
    if (!ctx || !ctx->finalized || !owner) return ADMM_ERR_ARG;
    for (int i = 0; i < ctx->n_nodes; ++i) owner[i] = (ctx->shard_mode == ADMM_SHARD_SUBTREE && ctx->world > 1) ? ctx->node_owner[ctx->F.iperm[i]] : 0;
    return ADMM_OK;
}
int admm_hip_debug_node_supernode(admm_hip_ctx *ctx, int32_t *supernode, int32_t *column, int32_t *parent) {
    if (!ctx || !ctx->finalized) return ADMM_ERR_ARG;
    const Factor &F = ctx->F;
    for (int s = 0; s < (int)F.sn.size(); ++s) {
        if (parent) parent[s] = F.sn[s].parent;
        for (int j = 0; j < F.sn[s].ncols; ++j) {
            const int i = F.perm[F.sn[s].first + j];
            if (supernode) supernode[i] = s;
            if (column) column[i] = j;
        }
    }
    return ADMM_OK;
}
#ifdef ADMM_TET_TIMELINE
// wave timeline of the NEXT tet launches (the buffer is overwritten by every launch: read it after the one of interest)
static unsigned long long *g_wave_t_buf; static size_t g_wave_t_n;
extern "C" int admm_hip_debug_tet_wave_times(long n_waves, unsigned long long *out) {
    if (!out) {      // arm
        hipFree(g_wave_t_buf); g_wave_t_buf = nullptr; g_wave_t_n = (size_t)n_waves;
        if (n_waves > 0 && hipMalloc(&g_wave_t_buf, 32 * g_wave_t_n) != hipSuccess) return ADMM_ERR_HIP;      // per wave: start, end, max evaluations, max iterations
        if (n_waves > 0) hipMemset(g_wave_t_buf, 0, 32 * g_wave_t_n);
        return hipMemcpyToSymbol(HIP_SYMBOL(admm_dev::g_tet_wave_t), &g_wave_t_buf, sizeof(g_wave_t_buf)) == hipSuccess ? ADMM_OK : ADMM_ERR_HIP;
    }
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, g_wave_t_buf, 32 * g_wave_t_n, hipMemcpyDeviceToHost) != hipSuccess) return ADMM_ERR_HIP;
    return ADMM_OK;
}
#endif
#ifdef ADMM_SWEEP_PROFILE
// -> stamps[4 * workgroups], meta[6 * launches]; returns the number of launches (negative: error; call with NULL for the sizes)
extern "C" long admm_hip_debug_sweep_profile_read(unsigned long long *stamps, int *meta) {
    if (!stamps) return (long)g_swp_wgs;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(stamps, g_swp_base, sizeof(unsigned long long) * 4 * g_swp_wgs, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (size_t i = 0; i < g_swp_meta.size(); ++i) meta[i] = g_swp_meta[i];
    return (long)(g_swp_meta.size() / 6);
}
#endif
#ifdef ADMM_TET_PROFILE
// tools/probe/ls_predict_gpu.py only (variant build): per-tet trace of the next `cap` launches of the tet kernel (0: off)
extern "C" int admm_hip_debug_tet_trace(int cap, int n) {
    hipFree(g_trace_base); g_trace_base = nullptr; g_trace_cap = cap; g_trace_n = n; g_trace_count = 0;
    if (cap > 0 && hipMalloc(&g_trace_base, sizeof(float) * 2 * (size_t)cap * n) != hipSuccess) return ADMM_ERR_HIP;
    return ADMM_OK;
}
extern "C" int admm_hip_debug_tet_trace_read(float *out) {
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, g_trace_base, sizeof(float) * 2 * (size_t)g_trace_cap * g_trace_n, hipMemcpyDeviceToHost) != hipSuccess) return ADMM_ERR_HIP;
    g_trace_count = 0;
    return ADMM_OK;
}
// tools/tet_phase_profile.py only (variant build): read and clear the tet kernel's phase counters
extern "C" int admm_hip_debug_tet_profile(unsigned long long *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(admm_dev::g_tet_prof), sizeof(unsigned long long) * 128) != hipSuccess) return ADMM_ERR_HIP;
    unsigned long long zero[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(admm_dev::g_tet_prof), zero, sizeof(zero)) != hipSuccess) return ADMM_ERR_HIP;
    return ADMM_OK;
}
#endif


static int check_pressure_chambers(admm_hip_ctx *ctx);      // (abi_pressure.inc)
static bool surface_reaction_any(const admm_hip_ctx *ctx);  // (abi_surface_reaction.inc)
static int surface_reaction_allocate(admm_hip_ctx *ctx);
static int rigid_allocate(admm_hip_ctx *ctx, int first_new);  // (abi_rigid.inc)
static bool attach_any(const admm_hip_ctx *ctx);              // (abi_attach.inc)
static int attach_upload(admm_hip_ctx *ctx);

int admm_hip_finalize(admm_hip_ctx *ctx) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "already finalized");
    if (ctx->dt <= 0.0) { fprintf(stderr, "\n**Solver Error: timestep set to %gs, changing to 0.04s.\n", ctx->dt); ctx->dt = 0.04; }
    if (ctx->n_nodes < 1 || ctx->m3.size() != ctx->x.size()) return fail(ctx, ADMM_ERR_ARG, "**Solver Error: Problem with node data!");
    std::fill(ctx->v.begin(), ctx->v.end(), 0.0); // System.cpp:113
    for (const Explicit &E : ctx->explicits) for (int32_t v : E.idx) if (v >= ctx->n_nodes) return fail(ctx, ADMM_ERR_ARG, "explicit force references node %d (have %d)", v, ctx->n_nodes);
    if (const char *e = getenv("ADMM_HIP_SHARD")) ctx->shard_mode = (std::string(e) == "subtree") ? ADMM_SHARD_SUBTREE : ADMM_SHARD_CONTIGUOUS;
    if (const char *g = getenv("ADMM_HIP_FACTOR_LOCAL")) ctx->factor_local = atoi(g) != 0;      // (overrides admm_hip_set_factor_local; host_factor picks the tree by it)
    TRY(check_body_entries(ctx, ctx->shapes.n, ctx->shapes.type, &ctx->shapes.par[0][0], true, ctx->shapes.mu, &ctx->shapes.motion[0][0], &ctx->shapes.frame[0][0]));
    for (int j = 0; j < ctx->shapes.n; ++j)
        if (!(ctx->shapes.mu[j] >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "collision shape %d: friction coefficient %g is negative or not a number", j, ctx->shapes.mu[j]);
    TRY(check_sheet_self_collision(ctx));
    TRY(check_body_self_collision(ctx));
    TRY(check_side_entries(ctx, ctx->shapes.n, ctx->shapes.type, &ctx->shapes.par[0][0]));
    TRY(check_pressure_chambers(ctx));
    // (belt and braces: admm_hip_set_shard refuses world > 1 above a share and admm_hip_set_surface_reaction refuses a share in a sharded
    //  context, so no sequence of calls reaches this today; it guards the step's launches against a later setter that forgets)
    if (ctx->world > 1 && surface_reaction_any(ctx))
        return fail(ctx, ADMM_ERR_UNSUPPORTED, "a surface reaction share is set in a sharded context (world = %d): a destination node may live on another rank", ctx->world);
    TRY(host_assemble(ctx, false));
    TRY(host_factor(ctx, false));
    ctx->info.rank = ctx->rank; ctx->info.world = ctx->world;
    if (ctx->dense) { ctx->shard_mode = 0; ctx->dist_top = false; }          // small systems: one-kernel solve, nothing to shard
    partition_subtrees(ctx);
    plan_device_panels(ctx);
    assign_elements(ctx);
    TRY(check_split_elements(ctx));
    shard_accounting(ctx);
    // Body surfaces under sharding need the full frame-start x on every rank; every mode has it, so none is refused: contiguous shards
    // all-reduce the whole right-hand side and solve the whole system on every rank, subtree shards (either top) rebuild the full x by
    // the masked all-reduce before the velocity update (shard_sync_x), and a dense solve is not sharded.  Every rank registers the same
    // surfaces and updates them from the same bits, so nothing of them goes over the collectives.
    const admm_lib::MeshTables plan = plan_context_meshes(ctx);      // (collision_plan.hpp; in device order, so behind host_factor)
    ctx->n_side_slots = plan.n_side_rows;                           // side memory: one row of sides per mesh with a reach
    for (size_t i = 0; i < ctx->meshes.size(); ++i) ctx->meshes[i].side_row = plan.side_row[i];
    if (ctx->device_id < 0) ctx->h_side.assign((size_t)ctx->n_side_slots * (size_t)ctx->n_nodes, 0);
    if (ctx->device_id >= 0) TRY(upload_all(ctx, plan));
    if (ctx->device_id >= 0 && ctx->attribution) { TRY(attribution_allocate(ctx)); TRY(attribution_fill(ctx)); }      // (switched on before finalize)
    if (ctx->device_id >= 0 && surface_reaction_any(ctx)) TRY(surface_reaction_allocate(ctx));      // (a share set before finalize)
    if (ctx->device_id >= 0 && !ctx->rigid.empty()) TRY(rigid_allocate(ctx, 0));      // (bodies registered before finalize)
    if (ctx->device_id >= 0 && attach_any(ctx)) TRY(attach_upload(ctx));      // (anchor batches attached before finalize)
    ctx->finalized = true;
    return ADMM_OK;
}
