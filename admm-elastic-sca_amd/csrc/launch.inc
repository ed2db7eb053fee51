// launch.inc -- one ADMM iteration as launches: local step (System.cpp:57-58), right-hand side (:61), the sweeps (:62), residuals
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)

int max_lbfgs_iters(const Batch &b) { return b.max_iter; }

// local step: every batch kernel on x_cur
#ifdef ADMM_TET_PROFILE
// tools/probe/ls_predict_gpu.py only (variant build): per-tet trace of the next `cap` launches of the tet kernel
float *g_trace_base; int g_trace_cap, g_trace_n, g_trace_count;
void tet_trace_next(hipStream_t st) {
    float *p = (g_trace_base && g_trace_count < g_trace_cap) ? g_trace_base + 2 * (size_t)g_trace_count * g_trace_n : nullptr;
    ++g_trace_count;
    hipMemcpyToSymbolAsync(HIP_SYMBOL(admm_dev::g_tet_trace), &p, sizeof(p), 0, hipMemcpyHostToDevice, st);
}
#endif
// which kernels the collision batches launch for the current list, and whether in a launch of their own (collision_plan.hpp: the forms 0
// to 7, their triggers, own_launch and sided; form 8 while contact attribution is on): one pass over the list, from the current
// coefficients, motions, frames and mesh records.
// Evaluated at every launch or capture, never kept: a setter changes it between frames, and the one that does drops the captured graphs
// (abi_setup.inc: push_shapes).  A form's kernel is an instantiation beside the others, not a flag inside them: a list that sets off no
// higher trigger launches exactly the kernels it launched before that form existed.
admm_lib::CollisionForm collision_form(const admm_hip_ctx *ctx) {
    return admm_lib::collision_form_of(ctx->shapes, (int)ctx->meshes.size(), [ctx](int id) {
        const admm_hip_ctx::CollisionMesh &m = ctx->meshes[id];
        return admm_lib::MeshFacts{m.body(), m.mesh.thickness, m.self_collision, m.side_reach, m.body_self[0], m.body_mu, m.has_vel};
    }, ctx->attribution);
}

// The scene's batches as segments of ONE project_multi_kernel launch (false: launch batch after batch -- a kind without a segment
// body, more than MULTI_MAX batches, or a tet batch with its anchors right behind it, which already is one launch).  own_launch: the
// collision batches stay out of the segments (collision_form)
bool build_multi(admm_hip_ctx *ctx, admm_dev::MultiBatch &mb, int &blocks, bool own_launch) {
    using namespace admm_dev;
    mb = MultiBatch{}; blocks = 0;
    // segments in the order of what a block costs, dearest first (the L-BFGS kinds, then the closed-form ones) whatever order the scene listed
    // its forces in (results do not depend on the order)
    auto dearness = [](int kind) {
        switch (kind) {
        case ADMM_KIND_TET_NH: return 0; case ADMM_KIND_TET_STVK: return 1; case ADMM_KIND_TRI_FUNG: return 2; case ADMM_KIND_TET_LINEAR: return 3; case ADMM_KIND_TET_VOLUME: return 4;
        case ADMM_KIND_BEND: return 5; case ADMM_KIND_TRI_STRAIN: return 6; case ADMM_KIND_TRI_AREA: return 7; case ADMM_KIND_SPRING: return 8; default: return 9;
        }
    };
    std::vector<const Batch *> seq;
    for (const Batch &b : ctx->batches) seq.push_back(&b);
    std::stable_sort(seq.begin(), seq.end(), [&](const Batch *a, const Batch *c) { return dearness(a->kind) < dearness(c->kind); });
    for (const Batch *bp : seq) {
        const Batch &b = *bp;
        if (b.n_local == 0 || b.kind == ADMM_KIND_GENERIC) continue;
        int code = -1;
        switch (b.kind) {
        case ADMM_KIND_TET_NH: code = max_lbfgs_iters(b) <= 5 ? MK_TET_NH : -1; break;
        case ADMM_KIND_TET_STVK: code = max_lbfgs_iters(b) <= 5 ? MK_TET_STVK : -1; break;
        case ADMM_KIND_TET_LINEAR: code = MK_TET_LINEAR; break;
        case ADMM_KIND_TET_VOLUME: code = MK_TET_VOLUME; break;
        case ADMM_KIND_ANCHOR: code = MK_ANCHOR; break;
        case ADMM_KIND_SPRING: code = MK_SPRING; break;
        case ADMM_KIND_BEND: code = MK_BEND; break;
        case ADMM_KIND_TRI_STRAIN: code = MK_TRI_STRAIN; break;
        case ADMM_KIND_TRI_AREA: code = MK_TRI_AREA; break;
        case ADMM_KIND_TRI_FUNG: code = MK_TRI_FUNG; break;
        case ADMM_KIND_COLLISION: if (own_launch) continue; code = MK_COLLISION; break;      // (meshes, friction, frames, boxes: own launch, launch_local)
        default: break;
        }
        if (code < 0 || mb.n == MULTI_MAX) return false;
        mb.b[mb.n] = batch_dev(ctx, b);
        blocks += batch_blocks(b);
        mb.code[mb.n] = code; mb.blk_end[mb.n] = blocks; ++mb.n;
    }
    if (mb.n < 2) return false;
    if (mb.n == 2 && mb.code[0] <= MK_TET_VOLUME && mb.code[1] == MK_ANCHOR && ctx->fuse_anchor_tail) {
        std::vector<int> live;      // ... in list order: the tail rides along only when the anchors come right behind their tets
        for (size_t bi = 0; bi < ctx->batches.size(); ++bi) if (ctx->batches[bi].n_local > 0 && ctx->batches[bi].kind != ADMM_KIND_GENERIC) live.push_back((int)bi);
        if (live.size() == 2 && live[1] == live[0] + 1 && ctx->batches[live[1]].kind == ADMM_KIND_ANCHOR) return false;
    }
    return true;
}

dim3 mesh_grid(int n) { return dim3((unsigned)((std::max(n, 1) + admm_dev::MESH_BLOCK - 1) / admm_dev::MESH_BLOCK)); }

// the commit of a mesh update (kernels_mesh.hpp), after the caller's check and volume stages: vertex normals, leaf slots, then the BVH
// refitted level by level from the deepest up.  gate: a body surface's verdict, read on the device (null: an obstacle, whose caller
// read the verdict back and comes here only to commit)
void launch_mesh_commit(const admm_hip_ctx::CollisionMesh &m, const int *gate, hipStream_t st) {
    using namespace admm_dev;
    using namespace admm_mesh;
    const admm_hip_mesh &M = m.mesh;
    const admm_hip_ctx::MeshUpdate &u = m.upd;
    const int nt = (int)M.tris.size(), nv = M.nv;
    hipLaunchKernelGGL(mesh_vertex_normal_kernel, mesh_grid(nv), dim3(MESH_BLOCK), 0, st, nv, (const double *)u.verts, (const int *)u.cid, (const double *)u.fn,
                       (const int *)u.inc_ptr, (const int *)u.inc, u.vn, gate);
    hipLaunchKernelGGL(mesh_slot_kernel, mesh_grid(nt), dim3(MESH_BLOCK), 0, st, nt, (const double *)u.verts, (const int *)u.cid, (const int *)u.adj,
                       (const double *)u.fn, (const double *)u.vn, u.tris, u.nrm, gate);
    for (int d = M.depth; d >= 0; --d) {
        const int n = M.lvl_ptr[d + 1] - M.lvl_ptr[d];
        hipLaunchKernelGGL(mesh_refit_kernel, mesh_grid(n), dim3(MESH_BLOCK), 0, st, (const int *)(u.lvl_nodes + M.lvl_ptr[d]), n, u.nodes, (const Tri *)u.tris, gate);
    }
}

// admm_hip_update_collision_mesh after finalize (kernels_mesh.hpp): check, refuse without touching the live arrays, or commit;
// synchronous on ctx->stream
int update_mesh_device(admm_hip_ctx *ctx, int id, const double *verts) {
    using namespace admm_dev;
    using namespace admm_mesh;
    const admm_hip_ctx::CollisionMesh &m = ctx->meshes[id];
    const admm_hip_mesh &M = m.mesh;
    const admm_hip_ctx::MeshUpdate &u = m.upd;
    const int nt = (int)M.tris.size(), nv = M.nv, nchunk = (nt + VOL_CHUNK - 1) / VOL_CHUNK;
    const hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(u.verts, verts, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ctx->d_mesh_chk, NO_TRI, 2, st));      // bad_tri = bad_vtx = none
    hipLaunchKernelGGL(mesh_check_kernel, mesh_grid(std::max(nt, nv)), dim3(MESH_BLOCK), 0, st, nt, nv, (const double *)u.verts, (const int *)u.cid, u.fn, u.part, ctx->d_mesh_chk);
    hipLaunchKernelGGL(mesh_volume_kernel, dim3(1), dim3(MESH_BLOCK), 0, st, nchunk, (const double *)u.part, ctx->d_mesh_chk, (BodyStatus *)nullptr, m.open() ? 1 : 0);
    UpdateCheck chk;
    HIPCHK(hipMemcpyAsync(&chk, ctx->d_mesh_chk, sizeof chk, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    char msg[512];
    if (mesh_refusal(M, verts, chk, msg, (int)sizeof msg)) return fail(ctx, ADMM_ERR_ARG, "collision mesh %d: %s", id, msg);
    launch_mesh_commit(m, nullptr, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return ADMM_OK;
}

// the frame-start update of every body surface (admm_hip_add_body_surface; kernels_mesh.hpp): the same stages as update_mesh_device
// from the frame-start x, eager on ctx->stream (outside the iteration and frame graphs), no read-back: the verdict gates the commit
// kernels on the device.  Every address was fixed at finalize.
int update_bodies(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    using namespace admm_mesh;
    const hipStream_t st = ctx->stream;
    for (const admm_hip_ctx::CollisionMesh &m : ctx->meshes) {
        const admm_hip_ctx::MeshUpdate &u = m.upd;
        if (!u.dnode) continue;
        const int nt = (int)m.mesh.tris.size(), nv = m.mesh.nv, nchunk = (nt + VOL_CHUNK - 1) / VOL_CHUNK;
        const int *gate = &u.status->gate;
        hipLaunchKernelGGL(mesh_gather_kernel, mesh_grid(nv), dim3(MESH_BLOCK), 0, st, nv, (const int *)u.dnode, (const double *)ctx->d_x, u.verts);
        hipLaunchKernelGGL(mesh_check_kernel, mesh_grid(std::max(nt, nv)), dim3(MESH_BLOCK), 0, st, nt, nv, (const double *)u.verts, (const int *)u.cid, u.fn, u.part, u.chk);
        hipLaunchKernelGGL(mesh_volume_kernel, dim3(1), dim3(MESH_BLOCK), 0, st, nchunk, (const double *)u.part, u.chk, u.status, m.open() ? 1 : 0);
        // the vertices' frame-start velocities beside them, through the same map (d_v before the explicit forces); gated like the commit
        // kernels: a refused frame keeps the velocities that went with the last good surface
        hipLaunchKernelGGL(mesh_gather_vel_kernel, mesh_grid(nv), dim3(MESH_BLOCK), 0, st, nv, (const int *)u.dnode, (const double *)ctx->d_v, m.d_vel, gate);
        launch_mesh_commit(m, gate, st);
    }
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// the device tables of the collision kernels (kernels_collision.hpp CollisionTables).  Every address was fixed at finalize; a table that
// the context does not have is null: the mesh tables without meshes, d_body_tag without an owner, d_mesh_self / d_self_vid without a
// self-colliding sheet (d_self_vid: or body), the side tables without a mesh with memory, d_mesh_bself / d_mesh_rest without a
// self-colliding body.  xs = the frame-start x: d_x is written by the epilogue only.
admm_dev::CollisionTables collision_tables(const admm_hip_ctx *ctx) {
    admm_dev::CollisionTables T{};
    T.xs = ctx->d_x; T.shapes = ctx->d_shapes; T.meshes = ctx->d_meshes; T.mm = ctx->d_mesh_motion; T.thick = ctx->d_mesh_thick; T.tag = ctx->d_body_tag;
    T.self = ctx->d_mesh_self; T.vid = ctx->d_self_vid;
    T.reach = ctx->d_mesh_reach; T.side_slot = ctx->d_mesh_side_slot; T.bnd = ctx->d_mesh_bnd; T.side = ctx->d_side; T.side_stride = ctx->n_nodes;
    T.bself = ctx->d_mesh_bself; T.rest = ctx->d_mesh_rest;
    T.dt = ctx->dt;
    return T;
}

// the latch of side memory (kernels_collision.hpp collision_side_kernel): every node's side on every mesh with memory that the current
// list names, from the frame-start x; eager on ctx->stream right after update_bodies (outside the iteration and frame graphs).  Every
// rank holds the full frame-start x, so every rank latches every node from the same bits.
int latch_sides(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    if (!ctx->d_side || !collision_form(ctx).sided) return ADMM_OK;      // (sided, not form >= 6: a self-colliding body named beside a mesh whose memory no entry names is form 7 without a latch)
    const int n = ctx->n_nodes;
    hipLaunchKernelGGL(collision_side_kernel, dim3((unsigned)((n + LOCAL_BLOCK - 1) / LOCAL_BLOCK)), dim3(LOCAL_BLOCK), 0, ctx->stream, collision_tables(ctx));
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// a collision batch of a context with mesh obstacles, friction, framed entries or boxes, or with contact attribution on: the kernel of
// the list's form.  (Forms 4 to 7 imply meshes; form 8 runs with and without; a body surface with a coefficient implies meshes and an
// entry's motion counts only beside its coefficient, so form 2 is reached.)
void launch_collision_mesh(admm_hip_ctx *ctx, const Batch &b, int form) {
    using namespace admm_dev;
    const BatchDev d = batch_dev(ctx, b);
    const dim3 grid((d.e1 - d.e0 + LOCAL_BLOCK - 1) / LOCAL_BLOCK), block(LOCAL_BLOCK);
    const double *x = ctx->d_xcur;
    CollisionTables T = collision_tables(ctx);
    const bool mesh = !ctx->meshes.empty();
    if (form == 8) { T.owner = ctx->d_at_owner + b.at_off; T.normal = ctx->d_at_normal + b.at_off; T.at_stride = ctx->at_total; }      // (allocated by the switch or by finalize)
#define ADMM_COLLIDE(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, ctx->stream, d, x, T)
    switch (form) {
    case 8: if (mesh) ADMM_COLLIDE(project_collision_attributed_kernel<true>); else ADMM_COLLIDE(project_collision_attributed_kernel<false>); break;
    case 7: ADMM_COLLIDE(project_collision_bodyself_kernel); break;
    case 6: ADMM_COLLIDE(project_collision_sided_kernel); break;
    case 5: ADMM_COLLIDE(project_collision_self_kernel); break;
    case 4: ADMM_COLLIDE(project_collision_shell_kernel); break;
    case 3: if (mesh) ADMM_COLLIDE(project_collision_framed_kernel<true>); else ADMM_COLLIDE(project_collision_framed_kernel<false>); break;
    case 2: if (mesh) ADMM_COLLIDE(project_collision_friction_moving_kernel<true>); else ADMM_COLLIDE(project_collision_friction_moving_kernel<false>); break;
    case 1: if (mesh) ADMM_COLLIDE(project_collision_friction_kernel<true>); else ADMM_COLLIDE(project_collision_friction_kernel<false>); break;
    default: ADMM_COLLIDE(project_collision_mesh_kernel); break;      // (form 0 in a launch of its own: own_launch, so the context has meshes)
    }
#undef ADMM_COLLIDE
}

int launch_local(admm_hip_ctx *ctx, int only_batch = -1, bool track = false) {
    using namespace admm_dev;
    hipStream_t const st = ctx->stream;
    const admm_lib::CollisionForm cf = collision_form(ctx);      // the current list, read once for every batch of this call
    // the whole local step in one launch: every batch a segment of project_multi_kernel's grid
    if (only_batch < 0 && !track && ctx->local_multi) {
        MultiBatch mb{}; int blocks = 0;
        if (build_multi(ctx, mb, blocks, cf.own_launch)) {
            hipLaunchKernelGGL(project_multi_kernel, dim3(blocks), dim3(LOCAL_BLOCK), 0, st, mb, (const double *)ctx->d_xcur, (const ShapeTable *)ctx->d_shapes);
            if (cf.own_launch)      // the collision batches were left out of the segments: their own launches
                for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_COLLISION && b.n_local > 0) launch_collision_mesh(ctx, b, cf.form);
            HIPCHK(hipGetLastError());
            return ADMM_OK;
        }
    }
    bool skip_next = false;
    for (size_t bi = 0; bi < ctx->batches.size(); ++bi) {
        const Batch &b = ctx->batches[bi];
        if (only_batch >= 0 && (int)bi != only_batch) continue;
        if (skip_next) { skip_next = false; continue; }                  // (an anchor batch that went out with the tets before it)
        if (b.n_local == 0 || b.kind == ADMM_KIND_GENERIC) continue;     // user-defined forces: generic_begin / generic_finish
        BatchDev d = batch_dev(ctx, b);
        const bool trk = track && b.res_fused;
        dim3 grid((d.e1 - d.e0 + b.tpb - 1) / b.tpb), block(LOCAL_BLOCK);
        const double *x = ctx->d_xcur;
        // an anchor batch right behind a tet batch rides along in the tet launch (project_tet_kernel's tail)
        BatchDev tail{}; const int tail_block0 = (int)grid.x;
        const bool is_tet = b.kind == ADMM_KIND_TET_NH || b.kind == ADMM_KIND_TET_STVK || b.kind == ADMM_KIND_TET_LINEAR || b.kind == ADMM_KIND_TET_VOLUME;
        // (with residual tracking only if both batches track inside their kernels: the tail runs the tet launch's TRACK variant)
        if (is_tet && only_batch < 0 && ctx->fuse_anchor_tail && bi + 1 < ctx->batches.size() && ctx->batches[bi + 1].kind == ADMM_KIND_ANCHOR && ctx->batches[bi + 1].n_local > 0 &&
            (!track || ctx->batches[bi + 1].res_fused == b.res_fused)) {
            tail = batch_dev(ctx, ctx->batches[bi + 1]);
            grid.x += (ctx->batches[bi + 1].n_local + LOCAL_BLOCK - 1) / LOCAL_BLOCK;
            skip_next = true;
        }
        switch (b.kind) {
        case ADMM_KIND_TET_NH:
#ifdef ADMM_TET_PROFILE
            tet_trace_next(st);
#endif
#define ADMM_TET(K, MM) do { if (trk) hipLaunchKernelGGL((project_tet_kernel<K, MM, true>), grid, block, 0, st, d, x, tail, tail_block0); \
                            else hipLaunchKernelGGL((project_tet_kernel<K, MM, false>), grid, block, 0, st, d, x, tail, tail_block0); } while (0)
            if (max_lbfgs_iters(b) <= 5) ADMM_TET(0, 5); else ADMM_TET(0, 10);
            break;
        case ADMM_KIND_TET_STVK:
            if (max_lbfgs_iters(b) <= 5) ADMM_TET(1, 5); else ADMM_TET(1, 10);
            break;
        case ADMM_KIND_TET_LINEAR: ADMM_TET(2, 1); break;
        case ADMM_KIND_TET_VOLUME: ADMM_TET(3, 1); break;
#undef ADMM_TET
        case ADMM_KIND_ANCHOR: if (trk) hipLaunchKernelGGL(project_anchor_kernel<true>, grid, block, 0, st, d, x); else hipLaunchKernelGGL(project_anchor_kernel<false>, grid, block, 0, st, d, x); break;
        case ADMM_KIND_SPRING: hipLaunchKernelGGL(project_spring_kernel, grid, block, 0, st, d, x); break;
        case ADMM_KIND_BEND: hipLaunchKernelGGL(project_bend_kernel, grid, block, 0, st, d, x); break;
        case ADMM_KIND_TRI_STRAIN: hipLaunchKernelGGL(project_tri_kernel<0>, grid, block, 0, st, d, x); break;
        case ADMM_KIND_TRI_AREA: hipLaunchKernelGGL(project_tri_kernel<1>, grid, block, 0, st, d, x); break;
        case ADMM_KIND_TRI_FUNG: hipLaunchKernelGGL(project_tri_kernel<2>, grid, block, 0, st, d, x); break;
        case ADMM_KIND_COLLISION:
            if (cf.own_launch) launch_collision_mesh(ctx, b, cf.form);
            else hipLaunchKernelGGL(project_collision_kernel, grid, block, 0, st, d, x, (const ShapeTable *)ctx->d_shapes);
            break;
        default: return fail(ctx, ADMM_ERR_UNSUPPORTED, "no kernel for kind %d", b.kind);
        }
    }
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// user-defined forces, first half: D_i x of the generic rows -> pinned host memory (asynchronous; the built-in kernels are
// launched behind it and run while the host projects)
int generic_begin(admm_hip_ctx *ctx, const double *x) {
    if (!ctx->n_gen_rows) return ADMM_OK;
    for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_GENERIC && b.g_lrows)
        hipLaunchKernelGGL(admm_dev::generic_dx_kernel, dim3((b.g_lrows + 255) / 256), dim3(256), 0, ctx->stream, b.g_lrows, (const int *)b.d_g_lrow, (const int *)b.d_g_rptr,
                           (const int *)b.d_g_col, (const double *)b.d_g_val, x, ctx->d_gen_dx);
    HIPCHK(hipMemcpyAsync(ctx->h_gen_dx, ctx->d_gen_dx, sizeof(double) * (size_t)ctx->n_gen_rows, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipEventRecord(ctx->gen_ev, ctx->stream));
    return ADMM_OK;
}
// second half: wait for the rows, run the caller's project() (Force::project for every user force, System.cpp:57-58),
// send z - u back and add the elements' shares of dt^2 D^T W^2 (z - u) to the per-node slots
int generic_finish(admm_hip_ctx *ctx) {
    if (!ctx->n_gen_rows) return ADMM_OK;
    HIPCHK(hipEventSynchronize(ctx->gen_ev));
    if (!ctx->project_hook) return fail(ctx, ADMM_ERR_STATE, "generic batches present but no project hook installed (admm_hip_set_project_hook)");
    if (ctx->project_hook(ctx->project_user, ctx->dt, ctx->n_gen_rows, ctx->h_gen_dx, ctx->h_gen_u, ctx->h_gen_z) != 0) return fail(ctx, ADMM_ERR_ARG, "project hook failed");
    for (int64_t r = 0; r < ctx->n_gen_rows; ++r) ctx->h_gen_q[r] = ctx->h_gen_z[r] - ctx->h_gen_u[r];
    HIPCHK(hipMemcpyAsync(ctx->d_gen_q, ctx->h_gen_q, sizeof(double) * (size_t)ctx->n_gen_rows, hipMemcpyHostToDevice, ctx->stream));
    for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_GENERIC && b.g_lslots)
        hipLaunchKernelGGL(admm_dev::generic_rhs_kernel, dim3((3 * b.g_lslots + 255) / 256), dim3(256), 0, ctx->stream, 3 * b.g_lslots, (const int *)b.d_g_sptr, (const int *)b.d_g_srow,
                           (const double *)b.d_g_scoef, (const int *)b.d_g_sdst, (const double *)ctx->d_gen_q, ctx->d_fslot);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

int launch_rhs(admm_hip_ctx *ctx) {
    const int n3 = 3 * ctx->n_nodes;
    if (n3 > 0) hipLaunchKernelGGL(admm_dev::rhs_gather_kernel<false>, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, 0, ctx->n_nodes, ctx->d_inc_ptr, ctx->slot_stride,
                                   ctx->d_fslot, ctx->d_mxbar, ctx->rank == 0 ? 1 : 0, (const unsigned char *)ctx->d_base_mask, ctx->d_y);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

// fn(std::integral_constant<int, V>) for the V among Vs that equals v: what fn returns, false where no V matches
template <int... Vs, class Fn> bool with_int(int v, Fn &&fn) { bool r = false; (void)((v == Vs && (r = fn(std::integral_constant<int, Vs>{}), true)) || ...); return r; }

// both triangular sweeps: d_y (rhs, destroyed) -> d_xcur
int launch_solve(admm_hip_ctx *ctx, hipEvent_t mid, hipEvent_t ex0 = nullptr, hipEvent_t ex1 = nullptr, hipEvent_t ex2 = nullptr, hipEvent_t ex3 = nullptr) {
    using namespace admm_dev;
    if (ctx->dense) {   // small system: one kernel, x = A_s^-1 b
        if (mid) HIPCHK(hipEventRecord(mid, ctx->stream));
        hipLaunchKernelGGL(dense_solve_kernel, dim3((ctx->n_nodes + 3) / 4), dim3(256), 0, ctx->stream, ctx->n_nodes, (const double *)ctx->d_ainv, (const double *)ctx->d_y, ctx->d_xcur);
        HIPCHK(hipGetLastError());
        return ADMM_OK;
    }
    const FactorDev F = factor_dev(ctx);
    // CG2: the children's contributions of every front row as fixed quadruples (F.cg4) rather than lists -- one choice for the whole solve
    auto sweeps = [&](auto cg2) -> int {
        constexpr bool CG2 = decltype(cg2)::value;
        auto forward = [&](const std::vector<LevelDev> &levels, hipStream_t st) {
            for (const LevelDev &L : levels) {
                if (L.n_small) hipLaunchKernelGGL((solve_fwd_small_kernel<CG2>), dim3((L.n_small + FWD_SMALL_WAVES - 1) / FWD_SMALL_WAVES), dim3(64 * FWD_SMALL_WAVES), 0, st, L.n_small, L.d_small, F, ctx->d_y, ctx->d_w, ctx->d_c);
                if (L.n_big) with_int<4, 8, 16>(L.big_nw, [&](auto nw) {
                    hipLaunchKernelGGL((solve_fwd_big_kernel<CG2, decltype(nw)::value>), dim3(L.n_big), dim3(64 * nw), 0, st, L.d_big, F, ctx->d_y, ctx->d_w, ctx->d_c); return true; });
                for (const LevelDev::Root &R : L.roots) {      // roots: both sweeps as one product with the explicit inverse, straight into x
                    const dim3 pg((R.k + ROOT_ROWS - 1) / ROOT_ROWS), pb(64 * ROOT_ROWS);
                    const double *Sinv = ctx->d_panels + R.inv_off;
                    double *Xr = ctx->d_xcur + 3 * (size_t)R.first;
                    if (R.k <= ctx->root_fuse_k) {      // small root: every block of the product gathers t itself (one launch less)
                        hipLaunchKernelGGL((root_product_kernel<true, CG2>), pg, pb, 0, st, R.k, R.k, root_inv_ld(R.k), Sinv, (const double *)ctx->d_y, Xr, R.first, R.foff, F, (const double *)ctx->d_c);
                        continue;
                    }
                    double *T = ctx->d_w + 3 * (size_t)R.first;      // the root's own slice of W is free: it has no backward launch
                    hipLaunchKernelGGL((root_gather_kernel<CG2>), dim3((R.k + 255) / 256), dim3(256), 0, st, R.k, R.first, R.foff, F, (const double *)ctx->d_y, (const double *)ctx->d_c, T);
                    hipLaunchKernelGGL((root_product_kernel<false, false>), pg, pb, 0, st, R.k, R.k, root_inv_ld(R.k), Sinv, (const double *)T, Xr, 0, (int64_t)0, F, (const double *)nullptr);
                }
            }
        };
        bool bad_pair = false;
        auto backward = [&](const std::vector<LevelDev> &levels, hipStream_t st) {
            for (int l = (int)levels.size() - 1; l >= 0; --l) {
                const LevelDev &L = levels[l];
                if (!L.n_bwd) continue;
                // the level's work items were cut for bwd_nw * bwd_cw columns per block (sweep_plan.hpp plan_levels): the kernel must be THAT pair
                // (two waves per block: four columns per wave only)
                bad_pair |= !with_int<4, 2, 1>(L.bwd_cw, [&](auto cw) { return with_int<2, 4, 8, 16>(L.bwd_nw, [&](auto nwb) {
                    constexpr int CW = decltype(cw)::value, NWB = decltype(nwb)::value;
                    if constexpr (NWB != 2 || CW == 4) hipLaunchKernelGGL((solve_bwd_kernel<CW, NWB>), dim3(L.n_bwd), dim3(64 * NWB), 0, st, L.d_bwd, F, ctx->d_w, ctx->d_xcur);
                    return NWB != 2 || CW == 4;
                }); });
            }
        };
        if (ctx->n_fuse)      // the bottom subtrees first, one workgroup each (then the levels above the cut)
            hipLaunchKernelGGL(solve_fwd_subtree_kernel, dim3(ctx->n_fuse), dim3(64 * SUB_WAVES), ctx->fuse_lds, ctx->stream, (const int *)ctx->d_fuse_rec,
                               (const int64_t *)ctx->d_fuse_off, (const double *)ctx->d_panels, (const double *)ctx->d_y, ctx->d_w, ctx->d_c);
        forward(ctx->levels, ctx->stream);
        if (!ctx->levels_top.empty()) {
            // subtree sharding: own subtrees are done; ONE small all-reduce carries the top nodes' partial right-hand sides and the
            // subtree roots' contributions to every rank, then everybody runs the (replicated) top of the tree
            const int n = ctx->n_comm_top + ctx->n_comm_slots;
            if (ex0) HIPCHK(hipEventRecord(ex0, ctx->stream));
            if (n > 0) {
                hipLaunchKernelGGL(shard_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_comm_top, (const int *)ctx->d_comm_top, ctx->n_comm_slots,
                                   (const int *)ctx->d_comm_slots, (const unsigned char *)ctx->d_comm_mine, (const double *)ctx->d_y, (const double *)ctx->d_c, ctx->d_comm_buf);
                TRY(do_allreduce(ctx, ctx->d_comm_buf, 3 * (int64_t)n));
                hipLaunchKernelGGL(shard_unpack_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_comm_top, (const int *)ctx->d_comm_top, ctx->n_comm_slots,
                                   (const int *)ctx->d_comm_slots, (const double *)ctx->d_comm_buf, ctx->d_y, ctx->d_c);
            }
            if (ex1) HIPCHK(hipEventRecord(ex1, ctx->stream));
            if (ctx->dist_top) {
                // distributed top: the root IS the top.  t = y - (the subtrees' contributions) on every rank (3 k doubles), then THIS rank's rows of
                // x = (L L^T)^-1 t straight into the root's range of x_cur, which the gather zeroed -- and a second small all-reduce (own rows + zeros: exact)
                // hands every rank the whole x of the top.  No replicated sweep over the top, no backward work above the own subtrees.
                const int k = ctx->root_k, nr = ctx->root_r1 - ctx->root_r0;
                double *T = ctx->d_w + 3 * (size_t)ctx->root_first, *Xr = ctx->d_xcur + 3 * (size_t)ctx->root_first;
                hipLaunchKernelGGL((root_gather_kernel<CG2>), dim3((k + 255) / 256), dim3(256), 0, ctx->stream, k, ctx->root_first, ctx->root_foff, F, (const double *)ctx->d_y, (const double *)ctx->d_c, T, Xr);
                if (nr > 0) hipLaunchKernelGGL((root_product_kernel<false, false>), dim3((nr + ROOT_ROWS - 1) / ROOT_ROWS), dim3(64 * ROOT_ROWS), 0, ctx->stream, k, nr, root_inv_ld(k),
                                               (const double *)(ctx->d_panels + ctx->dev_root_inv_off[ctx->root_sn]), (const double *)T, Xr + 3 * (size_t)ctx->root_r0, 0, (int64_t)0, F, (const double *)nullptr);
                if (ex2) HIPCHK(hipEventRecord(ex2, ctx->stream));
                TRY(do_allreduce(ctx, Xr, 3 * (int64_t)k));
                if (ex3) HIPCHK(hipEventRecord(ex3, ctx->stream));
            } else forward(ctx->levels_top, ctx->stream);
        }
        if (mid) HIPCHK(hipEventRecord(mid, ctx->stream));
        if (!ctx->levels_top.empty() && !ctx->dist_top) backward(ctx->levels_top, ctx->stream);
        backward(ctx->levels, ctx->stream);
        if (ctx->n_fuse_bwd)      // the bottom subtrees last, one workgroup each (bwd_small_nw: the block width of the per-level launches they replace)
            hipLaunchKernelGGL(solve_bwd_kernel_subtree, dim3(ctx->n_fuse_bwd), dim3(64 * SUB_WAVES), ctx->fuse_bwd_lds, ctx->stream, (const int *)ctx->d_fuse_bwd_rec,
                               (const int64_t *)ctx->d_fuse_bwd_off, (const double *)ctx->d_panels, (const double *)ctx->d_w, ctx->d_xcur, 4 * ctx->knobs.bwd_small_nw - 1);
        HIPCHK(hipGetLastError());
        if (bad_pair) return fail(ctx, ADMM_ERR_STATE, "backward sweep: no kernel for a level's (columns per wave, waves per block) pair");
        return ADMM_OK;
    };
    return F.cg4 ? sweeps(std::true_type{}) : sweeps(std::false_type{});
}

// subtree sharding: after the solve a rank holds x only on its own subtrees and the top; rebuild the full vector
// (once per frame, and for the solve-only entry point)
int shard_sync_x(admm_hip_ctx *ctx) {
    if (ctx->levels_top.empty()) return ADMM_OK;
    const int n3 = 3 * ctx->n_nodes;
    hipLaunchKernelGGL(admm_dev::shard_mask_nodes_kernel, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_nodes, (const unsigned char *)ctx->d_keep_mask, ctx->d_xcur);
    TRY(do_allreduce(ctx, ctx->d_xcur, (int64_t)n3));
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}


// ---- residual tracking (opt-in): buffers are created on first use -------------------------------------
int ensure_residual_buffers(admm_hip_ctx *ctx, int iters) {
    if (ctx->res_ready && iters <= ctx->res_cap) return ADMM_OK;
    HIPCHK(hipSetDevice(ctx->device_id));
    if (!ctx->res_ready) {
        int64_t slots = 0; int maxn = 0;
        for (Batch &b : ctx->batches) {
            if (b.kind == ADMM_KIND_GENERIC) {      // user rows: u, z live on the host; the dual residual goes through the same slots with w^2 coefficients
                std::vector<double> coef(b.g_sval.size());
                for (size_t i = 0; i < coef.size(); ++i) { const double w = b.g_roww[b.g_srow_b[i]]; coef[i] = b.g_sval[i] * (w * w); }
                TRY(upload(ctx, &b.d_g_scoef_res, coef));
                slots += b.g_lslots;
                continue;
            }
            const int rows = ADMM_KIND_ROWS[b.kind], nl = std::max(b.n_local, 1);
            // (ADMM_HIP_RES_UNFUSED=1: the separate passes, for comparison; not for pre-reduced tet batches, which have no per-corner slots)
            b.res_fused = ((b.kind >= ADMM_KIND_TET_LINEAR && b.kind <= ADMM_KIND_TET_STVK) || b.kind == ADMM_KIND_ANCHOR) && (b.prered || getenv("ADMM_HIP_RES_UNFUSED") == nullptr);
            if (b.res_fused) {      // the tet kernels produce their residuals themselves: no snapshots, one partial per 64-tet block
                const int nblk = std::max(batch_blocks(b), 1);
                TRY(dalloc(ctx, &b.d_res_partial, (size_t)nblk));
                HIPCHK(hipMemsetAsync(b.d_res_partial, 0, sizeof(double) * (size_t)nblk, ctx->stream));      // (stream-ordered: on a caller's non-blocking stream the default stream orders nothing)
            } else { TRY(dalloc(ctx, &b.d_u_prev, (size_t)rows * nl)); TRY(dalloc(ctx, &b.d_z_prev, (size_t)rows * nl)); }
            TRY(upload(ctx, &b.d_G, b.G));
            slots += (int64_t)b.n_local * ADMM_KIND_NODES[b.kind]; maxn = std::max(maxn, b.n_local);
        }
        if (ctx->n_gen_rows) {
            ctx->h_gen_u_prev.assign((size_t)ctx->n_gen_rows, 0.0); ctx->h_gen_z_prev.assign((size_t)ctx->n_gen_rows, 0.0);
            TRY(dalloc(ctx, &ctx->d_gen_q2, (size_t)ctx->n_gen_rows)); TRY(dalloc(ctx, &ctx->d_gen_r2, 1));
        }
        slots = std::max<int64_t>(slots, ctx->n_fslots);      // same layout as the RHS slots
        TRY(dalloc(ctx, &ctx->d_res_slots, 3 * (size_t)std::max<int64_t>(slots, 1)));
        HIPCHK(hipMemsetAsync(ctx->d_res_slots, 0, sizeof(double) * 3 * (size_t)std::max<int64_t>(slots, 1), ctx->stream));
        TRY(dalloc(ctx, &ctx->d_res_s, 3 * (size_t)ctx->n_nodes));
        ctx->res_partial_n = std::max((maxn + admm_dev::RES_BLOCK - 1) / admm_dev::RES_BLOCK, (3 * ctx->n_nodes + admm_dev::RES_BLOCK - 1) / admm_dev::RES_BLOCK);
        TRY(dalloc(ctx, &ctx->d_res_partial, (size_t)std::max(ctx->res_partial_n, 1)));
        ctx->res_ready = true; ctx->res_cap = 0;
    }
    if (iters > ctx->res_cap) { ctx->res_cap = std::max(iters, 64); TRY(dalloc(ctx, &ctx->d_res, 2 * (size_t)ctx->res_cap)); }
    return ADMM_OK;
}
// before the local step: keep u and z of the previous iteration
int residual_snapshot(admm_hip_ctx *ctx, bool first_iteration) {
    if (ctx->n_gen_rows) {      // user rows (host): at a frame's first iteration h_gen_z already holds D * m_x (admm_hip_step)
        std::memcpy(ctx->h_gen_u_prev.data(), ctx->h_gen_u, sizeof(double) * (size_t)ctx->n_gen_rows);
        std::memcpy(ctx->h_gen_z_prev.data(), ctx->h_gen_z, sizeof(double) * (size_t)ctx->n_gen_rows);
    }
    for (Batch &b : ctx->batches) {
        if (!b.n_local || b.kind == ADMM_KIND_GENERIC) continue;
        const int rows = ADMM_KIND_ROWS[b.kind];
        if (b.res_fused) {     // z_prev is the kernel's own previous output; only the frame's warm start has to be put there
            if (first_iteration)
                hipLaunchKernelGGL(admm_dev::residual_dx_kernel, dim3((b.n_local + admm_dev::RES_BLOCK - 1) / admm_dev::RES_BLOCK), dim3(admm_dev::RES_BLOCK), 0, ctx->stream,
                                   b.n_local, ADMM_KIND_NODES[b.kind], rows / 3, idx_stride(b.kind), b.d_idx, b.d_G, ctx->d_x, b.d_z);
            continue;
        }
        const int64_t cnt = (int64_t)rows * b.n_local;      // one launch instead of two device-to-device copies (each a ~10 us operation whatever its size)
        hipLaunchKernelGGL(admm_dev::residual_snapshot_kernel, dim3((unsigned)((cnt + admm_dev::RES_BLOCK - 1) / admm_dev::RES_BLOCK)), dim3(admm_dev::RES_BLOCK), 0, ctx->stream,
                           cnt, (const double *)b.d_u, (const double *)b.d_z, b.d_u_prev, b.d_z_prev, first_iteration ? 0 : 1);
        if (first_iteration)   // the reference warm-starts curr_z = D * m_x before the loop (System.cpp:43)
            hipLaunchKernelGGL(admm_dev::residual_dx_kernel, dim3((b.n_local + admm_dev::RES_BLOCK - 1) / admm_dev::RES_BLOCK), dim3(admm_dev::RES_BLOCK), 0, ctx->stream,
                               b.n_local, ADMM_KIND_NODES[b.kind], rows / 3, idx_stride(b.kind), b.d_idx, b.d_G, ctx->d_x, b.d_z_prev);
    }
    return ADMM_OK;
}
// after the local step: d_res[2 it] = |r|^2 (this rank's elements), d_res[2 it + 1] = |s|^2
int launch_residuals(admm_hip_ctx *ctx, int it) {
    using namespace admm_dev;
    const int n3 = 3 * ctx->n_nodes;
    double *r2 = ctx->d_res + 2 * (size_t)it, *s2 = r2 + 1;
    bool first = true;
    if (ctx->n_gen_rows) {      // user rows: |r|^2 of this rank's rows on the host, z - z_prev to the device for the dual residual
        double r2h = 0.0;
        for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_GENERIC)
            for (int el = 0; el < b.n_local; ++el) for (int64_t r = b.g_elem_row[b.local[el]]; r < b.g_elem_row[b.local[el] + 1]; ++r) {
                const double d = ctx->h_gen_u[b.g_row0 + r] - ctx->h_gen_u_prev[b.g_row0 + r], w = b.g_roww[r];
                r2h += (w * w) * (d * d);
            }
        HIPCHK(hipStreamSynchronize(ctx->stream));      // h_gen_q may still be the source of generic_finish's asynchronous upload
        for (int64_t r = 0; r < ctx->n_gen_rows; ++r) ctx->h_gen_q[r] = ctx->h_gen_z[r] - ctx->h_gen_z_prev[r];
        HIPCHK(hipMemcpyAsync(ctx->d_gen_q2, ctx->h_gen_q, sizeof(double) * (size_t)ctx->n_gen_rows, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->d_gen_r2, &r2h, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));      // (r2h is a stack variable)
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(RES_BLOCK), 0, ctx->stream, 1, (const double *)ctx->d_gen_r2, r2, 0);
        first = false;
        for (const Batch &b : ctx->batches) if (b.kind == ADMM_KIND_GENERIC && b.g_lslots)
            hipLaunchKernelGGL(generic_rhs_kernel, dim3((3 * b.g_lslots + 255) / 256), dim3(256), 0, ctx->stream, 3 * b.g_lslots, (const int *)b.d_g_sptr, (const int *)b.d_g_srow,
                               (const double *)b.d_g_scoef_res, (const int *)b.d_g_sdst, (const double *)ctx->d_gen_q2, ctx->d_res_slots);
    }
    for (Batch &b : ctx->batches) {
        if (!b.n_local || b.kind == ADMM_KIND_GENERIC) continue;
        if (b.res_fused) {     // |r|^2 partials and the s slots were written by the projection kernel
            const int nblk = batch_blocks(b);
            hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(RES_BLOCK), 0, ctx->stream, nblk, (const double *)b.d_res_partial, r2, first ? 0 : 1);
            first = false;
            continue;
        }
        const int nb = (b.n_local + RES_BLOCK - 1) / RES_BLOCK, rows = ADMM_KIND_ROWS[b.kind];
        hipLaunchKernelGGL(residual_primal_kernel, dim3(nb), dim3(RES_BLOCK), 0, ctx->stream, b.n_local, rows, b.d_u, b.d_u_prev, b.d_w2, ctx->d_res_partial);
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(RES_BLOCK), 0, ctx->stream, nb, ctx->d_res_partial, r2, first ? 0 : 1);
        hipLaunchKernelGGL(residual_dual_kernel, dim3(nb), dim3(RES_BLOCK), 0, ctx->stream, b.n_local, ADMM_KIND_NODES[b.kind], rows / 3, idx_stride(b.kind),
                           b.d_z, b.d_z_prev, b.d_w2, b.d_G, b.d_dst, ctx->d_res_slots);
        first = false;
    }
    if (first) HIPCHK(hipMemsetAsync(r2, 0, sizeof(double), ctx->stream));
    const int nb = (n3 + RES_BLOCK - 1) / RES_BLOCK;
    static_assert(RES_BLOCK == 256, "the gather's blocks are the norm's partials");
    if (ctx->world == 1) {      // one rank: the gather of s leaves its blocks' sums of squares behind, no norm pass
        hipLaunchKernelGGL(rhs_gather_kernel<true>, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, 0, ctx->n_nodes, ctx->d_inc_ptr, ctx->slot_stride, ctx->d_res_slots, ctx->d_mxbar, 0, (const unsigned char *)nullptr, ctx->d_res_s, ctx->d_res_partial);
    } else {                    // s is a sum over all ranks' elements (all-reduced before its norm); r^2 is additive
        hipLaunchKernelGGL(rhs_gather_kernel<false>, dim3((n3 + 255) / 256), dim3(256), 0, ctx->stream, 0, ctx->n_nodes, ctx->d_inc_ptr, ctx->slot_stride, ctx->d_res_slots, ctx->d_mxbar, 0, (const unsigned char *)nullptr, ctx->d_res_s);
        if (ctx->world > 1) { TRY(do_allreduce(ctx, ctx->d_res_s, (int64_t)n3)); TRY(do_allreduce(ctx, r2, 1)); }
        hipLaunchKernelGGL(norm2_partial_kernel, dim3(nb), dim3(RES_BLOCK), 0, ctx->stream, n3, ctx->d_res_s, ctx->d_res_partial);
    }
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(RES_BLOCK), 0, ctx->stream, nb, ctx->d_res_partial, s2, 0);
    HIPCHK(hipGetLastError());
    return ADMM_OK;
}

int require_device(admm_hip_ctx *ctx) {
    if (!ctx) return ADMM_ERR_ARG;
    if (ctx->device_id < 0) return fail(ctx, ADMM_ERR_HIP, "host-only context: no GPU path available (the product has no CPU fallback)");
    if (!ctx->finalized) return fail(ctx, ADMM_ERR_STATE, "admm_hip_finalize has not been called");
    return ADMM_OK;
}

int require_factor(admm_hip_ctx *ctx) {
    TRY(require_device(ctx));
    if (ctx->factor_invalid) return fail(ctx, ADMM_ERR_STATE, "no valid factorization: the last recompute_weights failed (%s); a recompute_weights that succeeds restores it", ctx->factor_error.c_str());
    return ADMM_OK;
}
