// abi_rigid.inc -- C ABI: rigid bodies in the collision list, moved by the reaction of their contacts (kernels_rigid.hpp, rigid.hpp), and
// the launches admm_hip_step makes for them: the pose at its very start, the integration between its epilogue (and the two-way contact)
// and the velocity damping
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)
// Extension, no reference counterpart.  The launches write the bodies' records, their entries' rows of the shape table and the buffers of
// the reaction and attribution reports (abi_reaction.inc), nothing else of the solver's state; they run eagerly on the context's stream,
// outside the captured iteration and frame graphs, and drop none of them.  A context without a body launches and uploads nothing here.

static int launch_attach_targets(admm_hip_ctx *ctx);      // (abi_attach.inc)
static int launch_attach_load(admm_hip_ctx *ctx);

static int body_of_entry(const admm_hip_ctx *ctx, int entry) {
    for (size_t b = 0; b < ctx->rigid.size(); ++b) if (ctx->rigid[b].K.entry == entry) return (int)b;
    return -1;
}

// the host's shape table rows of body b, from the host's copy of its record
static void rigid_mirror_pose(admm_hip_ctx *ctx, int b) {
    const admm_hip_ctx::RigidBodyHost &B = ctx->rigid[b];
    const int e = B.K.entry;
    ctx->shapes.framed[e] = admm_rigid::pose(B.rec, ctx->shapes.par[e], ctx->shapes.frame[e], ctx->shapes.motion[e]);
}

static admm_dev::RigidTable rigid_table(const admm_hip_ctx *ctx) {
    admm_dev::RigidTable T{};
    T.n = (int)ctx->rigid.size();
    for (int &r : T.body_of_row) r = -1;
    for (int b = 0; b < T.n; ++b) { T.K[b] = ctx->rigid[b].K; T.body_of_row[T.K[b].entry] = b; }
    return T;
}

// every buffer the frame's launches need, the reaction and attribution reports' included, and the table and the records as the host
// holds them; a finalized device context with contact attribution on.  first_new: the records from that body on are uploaded (the
// earlier ones live on the device)
static int rigid_allocate(admm_hip_ctx *ctx, int first_new) {
    using namespace admm_dev;
    HIPCHK(hipSetDevice(ctx->device_id));
    TRY(attribution_allocate(ctx));
    TRY(ensure_attribution_buffers(ctx));
    if (!ctx->d_rg_table) { RigidTable *t = nullptr; TRY(dalloc(ctx, &t, 1)); ctx->d_rg_table = t; }
    if (!ctx->d_rg_rec) { admm_rigid::Record *r = nullptr; TRY(dalloc(ctx, &r, (size_t)ADMM_MAX_SHAPES)); ctx->d_rg_rec = r; HIPCHK(hipMemset(r, 0, sizeof(admm_rigid::Record) * ADMM_MAX_SHAPES)); }
    if (!ctx->d_rg_out) { TRY(dalloc(ctx, &ctx->d_rg_out, 6 * (size_t)ADMM_MAX_SHAPES)); HIPCHK(hipMemset(ctx->d_rg_out, 0, sizeof(double) * 6 * ADMM_MAX_SHAPES)); }
    HIPCHK(hipStreamSynchronize(ctx->stream));      // (the frames queued so far read the table as it was)
    const RigidTable T = rigid_table(ctx);
    HIPCHK(hipMemcpy(ctx->d_rg_table, &T, sizeof T, hipMemcpyHostToDevice));
    for (size_t b = (size_t)first_new; b < ctx->rigid.size(); ++b) {
        HIPCHK(hipMemcpy((admm_rigid::Record *)ctx->d_rg_rec + b, &ctx->rigid[b].rec, sizeof(admm_rigid::Record), hipMemcpyHostToDevice));
        ctx->rigid[b].accel_dirty = false;
    }
    ctx->rg_ready = true;
    return ADMM_OK;
}

// admm_hip_step, before update_bodies and latch_sides: the pose of every body into its entry's rows of the shape table
static int launch_rigid_pose(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    if (!ctx->rg_ready) return fail(ctx, ADMM_ERR_STATE, "rigid bodies: a body is registered but the buffers were never allocated");
    RigidTable *T = (RigidTable *)ctx->d_rg_table;
    for (size_t b = 0; b < ctx->rigid.size(); ++b) {      // (the accelerations travel as kernel arguments: no host buffer has to outlive the call)
        admm_hip_ctx::RigidBodyHost &B = ctx->rigid[b];
        if (!B.accel_dirty) continue;
        hipLaunchKernelGGL(rigid_set_accel_kernel, dim3(1), dim3(RIGID_BLOCK), 0, ctx->stream, T, (int)b, B.K.accel[0], B.K.accel[1], B.K.accel[2]);
        B.accel_dirty = false;
    }
    hipLaunchKernelGGL(rigid_pose_kernel, dim3(1), dim3(RIGID_BLOCK), 0, ctx->stream, (const RigidTable *)T, (const admm_rigid::Record *)ctx->d_rg_rec, ctx->d_shapes);
    HIPCHK(hipGetLastError());
    if (ctx->att_slots) TRY(launch_attach_targets(ctx));      // rigid attachments (abi_attach.inc): the attached batches' targets from the same records
    return ADMM_OK;
}

// admm_hip_step, behind epilogue_kernel and launch_surface_reaction, before the damping filter
static int launch_rigid_integrate(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    if (!ctx->rg_ready) return fail(ctx, ADMM_ERR_STATE, "rigid bodies: a body is registered but the buffers were never allocated");
    const double depth_min = ctx->rg_depth_min;
    // the contacts of admm_hip_entry_resultants(depth_min) and their owners, sorted by entry, by the reports' own launches
    TRY(launch_contact_chain(ctx, depth_min, CHAIN_RECORDS | CHAIN_OWNERS | CHAIN_SORTED));
    const EntryWork W = entry_work(ctx, true);
    const int nb = (int)ctx->rigid.size();
    const long long *total = W.totals;
    const RigidTable *T = (const RigidTable *)ctx->d_rg_table;
    admm_rigid::Record *rec = (admm_rigid::Record *)ctx->d_rg_rec;
    hipLaunchKernelGGL(rigid_partial_kernel, dim3(W.nblk + W.rows), dim3(ENERGY_BLOCK), 0, ctx->stream, (const ContactRecord *)ctx->d_rx_rec, (const int *)W.perm, W.rows, total, T,
                       (const admm_rigid::Record *)rec, W.n_part, W.partials);
    hipLaunchKernelGGL(rigid_reduce_kernel, dim3(6 * nb), dim3(ENERGY_REDUCE), 0, ctx->stream, T, total, W.n_part, (const double *)W.partials, ctx->d_rg_out);
    if (ctx->att_slots) TRY(launch_attach_load(ctx));      // rigid attachments (abi_attach.inc): what the bodies carry, added to their rows
    hipLaunchKernelGGL(rigid_integrate_kernel, dim3(1), dim3(RIGID_BLOCK), 0, ctx->stream, T, total, (const double *)ctx->d_rg_out, ctx->dt, rec);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

static bool rigid_finite3(const double *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

int admm_hip_add_rigid_body(admm_hip_ctx *ctx, int entry, double mass, const double inertia[6], const double com[3], const double accel[3], int *body_id) {
    if (!ctx || !inertia || !com) return ADMM_ERR_ARG;
    if (entry < 0 || entry >= ctx->shapes.n) return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d is not an entry of the collision list (%d entries)", entry, ctx->shapes.n);
    if (body_of_entry(ctx, entry) >= 0) return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d is a rigid body already (body %d)", entry, body_of_entry(ctx, entry));
    const int type = ctx->shapes.type[entry];
    if (type == ADMM_SHAPE_FLOOR || type == ADMM_SHAPE_CYLINDER)
        return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d is a %s, an infinite shape: it cannot be a rigid body", entry, type == ADMM_SHAPE_FLOOR ? "floor" : "cylinder");
    const admm_hip_ctx::CollisionMesh *m = entry_mesh(ctx, ctx->shapes.type, &ctx->shapes.par[0][0], entry);
    if (m && m->body())
        return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d names mesh %d, a body or sheet surface: it follows its simulated nodes", entry, (int)ctx->shapes.par[entry][3]);
    admm_hip_ctx::RigidBodyHost B{};
    if (!(mass > 0.0) || !std::isfinite(mass)) return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d: mass %g: it must be positive and finite", entry, mass);
    if (!rigid_finite3(com) || (accel && !rigid_finite3(accel))) return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d: the centre of mass or the acceleration is not finite", entry);
    if (!admm_rigid::invert_inertia(inertia, B.K.Jinv))
        return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d: the inertia tensor (%g, %g, %g, %g, %g, %g) is not finite or not positive definite", entry, inertia[0], inertia[1], inertia[2],
                    inertia[3], inertia[4], inertia[5]);
    if (!ctx->attribution)
        return fail(ctx, ADMM_ERR_STATE, "add_rigid_body: entry %d: contact attribution is off (admm_hip_enable_contact_attribution): a body's load needs every contact's owner entry", entry);
    if (ctx->world > 1)
        return fail(ctx, ADMM_ERR_UNSUPPORTED, "add_rigid_body: entry %d: not available in a sharded context (world = %d): a rank sees only its share of the contacts", entry, ctx->world);
    const double *f = ctx->shapes.frame[entry];
    const bool at_com = f[9] == com[0] && f[10] == com[1] && f[11] == com[2];
    if (type == ADMM_SHAPE_BOX && !at_com)
        return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d is a box, whose centre is its frame's pivot (%g, %g, %g): the centre of mass (%g, %g, %g) must be that point", entry, f[9], f[10],
                    f[11], com[0], com[1], com[2]);
    if (!admm_frame::identity(f) && !at_com)
        return fail(ctx, ADMM_ERR_ARG, "add_rigid_body: entry %d: its frame turns it about (%g, %g, %g), not about the centre of mass (%g, %g, %g): pivot the frame at the centre of mass", entry,
                    f[9], f[10], f[11], com[0], com[1], com[2]);
    B.K.mass = mass; B.K.entry = entry; B.K.type = type;
    for (int j = 0; j < 6; ++j) B.inertia[j] = inertia[j];
    for (int j = 0; j < 3; ++j) { B.K.accel[j] = accel ? accel[j] : 0.0; B.K.c0[j] = com[j]; B.rec.c[j] = com[j]; B.rec.v[j] = 0.0; B.rec.L[j] = 0.0; }
    for (int j = 0; j < 4; ++j) B.K.par0[j] = ctx->shapes.par[entry][j];
    admm_rigid::quaternion_of(f, B.rec.q);
    admm_rigid::derive(B.K, B.rec);
    ctx->rigid.push_back(B);
    const int b = (int)ctx->rigid.size() - 1;
    if (ctx->finalized && ctx->device_id >= 0) {      // (before finalize: finalize does it)
        const int rc = rigid_allocate(ctx, b);
        if (rc) { ctx->rigid.pop_back(); return rc; }
    }
    rigid_mirror_pose(ctx, b);
    if (body_id) *body_id = b;
    return ADMM_OK;
}

int admm_hip_set_rigid_depth(admm_hip_ctx *ctx, double depth_min) {
    if (!ctx) return ADMM_ERR_ARG;
    if (!(depth_min >= 0.0)) return fail(ctx, ADMM_ERR_ARG, "set_rigid_depth: depth_min must be >= 0, got %g", depth_min);
    ctx->rg_depth_min = depth_min;
    return ADMM_OK;
}

int admm_hip_get_rigid_state(admm_hip_ctx *ctx, int n_bodies, admm_hip_rigid_state *out) {
    if (!ctx) return ADMM_ERR_ARG;
    if (n_bodies != (int)ctx->rigid.size() || (n_bodies && !out)) return fail(ctx, ADMM_ERR_ARG, "get_rigid_state: %d records given, the context has %d rigid bodies", n_bodies, (int)ctx->rigid.size());
    static_assert(sizeof(admm_hip_rigid_state) == sizeof(admm_rigid::Record), "admm_hip_rigid_state is the device's record");
    if (n_bodies && ctx->rg_ready) {
        HIPCHK(hipSetDevice(ctx->device_id));
        std::vector<admm_rigid::Record> h((size_t)n_bodies);
        HIPCHK(hipMemcpyAsync(h.data(), ctx->d_rg_rec, sizeof(admm_rigid::Record) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int b = 0; b < n_bodies; ++b) { ctx->rigid[b].rec = h[b]; rigid_mirror_pose(ctx, b); }
    }
    for (int b = 0; b < n_bodies; ++b) std::memcpy(out + b, &ctx->rigid[b].rec, sizeof(admm_rigid::Record));
    return ADMM_OK;
}

int admm_hip_set_rigid_state(admm_hip_ctx *ctx, int body, const double c[3], const double q[4], const double v[3], const double L[3]) {
    if (!ctx || !c || !q || !v || !L) return ADMM_ERR_ARG;
    if (body < 0 || body >= (int)ctx->rigid.size()) return fail(ctx, ADMM_ERR_ARG, "set_rigid_state: body %d is not a rigid body (have %d)", body, (int)ctx->rigid.size());
    admm_hip_ctx::RigidBodyHost &B = ctx->rigid[body];
    admm_rigid::Record R = B.rec;
    if (!rigid_finite3(c) || !rigid_finite3(v) || !rigid_finite3(L) || !admm_rigid::accept_quaternion(q, R.q))
        return fail(ctx, ADMM_ERR_ARG, "set_rigid_state: body %d (entry %d): a value is not finite, or the quaternion is zero", body, B.K.entry);
    for (int j = 0; j < 3; ++j) { R.c[j] = c[j]; R.v[j] = v[j]; R.L[j] = L[j]; }
    admm_rigid::derive(B.K, R);
    if (ctx->rg_ready) {
        HIPCHK(hipSetDevice(ctx->device_id));
        HIPCHK(hipMemcpyAsync((admm_rigid::Record *)ctx->d_rg_rec + body, &R, sizeof R, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    B.rec = R;
    rigid_mirror_pose(ctx, body);
    return ADMM_OK;
}

int admm_hip_set_rigid_accel(admm_hip_ctx *ctx, int body, const double accel[3]) {
    if (!ctx || !accel) return ADMM_ERR_ARG;
    if (body < 0 || body >= (int)ctx->rigid.size()) return fail(ctx, ADMM_ERR_ARG, "set_rigid_accel: body %d is not a rigid body (have %d)", body, (int)ctx->rigid.size());
    if (!rigid_finite3(accel)) return fail(ctx, ADMM_ERR_ARG, "set_rigid_accel: body %d (entry %d): the acceleration is not finite", body, ctx->rigid[body].K.entry);
    admm_hip_ctx::RigidBodyHost &B = ctx->rigid[body];
    for (int j = 0; j < 3; ++j) B.K.accel[j] = accel[j];
    B.accel_dirty = true;      // (reaches the device with the next step's launches)
    return ADMM_OK;
}

int admm_hip_get_rigid_body(admm_hip_ctx *ctx, int body, int *entry, int *type, double *mass, double inertia[6], double accel[3], double c0[3], double par0[4]) {
    if (!ctx) return ADMM_ERR_ARG;
    if (body < 0 || body >= (int)ctx->rigid.size()) return fail(ctx, ADMM_ERR_ARG, "get_rigid_body: body %d is not a rigid body (have %d)", body, (int)ctx->rigid.size());
    const admm_hip_ctx::RigidBodyHost &B = ctx->rigid[body];
    if (entry) *entry = B.K.entry;
    if (type) *type = B.K.type;
    if (mass) *mass = B.K.mass;
    if (inertia) for (int j = 0; j < 6; ++j) inertia[j] = B.inertia[j];
    if (accel) for (int j = 0; j < 3; ++j) accel[j] = B.K.accel[j];
    if (c0) for (int j = 0; j < 3; ++j) c0[j] = B.K.c0[j];
    if (par0) for (int j = 0; j < 4; ++j) par0[j] = B.K.par0[j];
    return ADMM_OK;
}
