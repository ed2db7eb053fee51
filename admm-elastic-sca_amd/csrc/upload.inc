// upload.inc -- the factor and the batches on the device: the sweeps' plan (sweep_plan.hpp) printed and uploaded, SoA element arrays, RHS slot layout
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)

// ---- device upload ----------------------------------------------------------
template <class T> std::vector<T> permute_nodes(const std::vector<T> &h, const std::vector<int> &perm, int comps) {
    std::vector<T> o(h.size());
    for (size_t i = 0; i < perm.size(); ++i) for (int c = 0; c < comps; ++c) o[comps * i + c] = h[comps * (size_t)perm[i] + c];
    return o;
}

#ifdef ADMM_SWEEP_PROFILE
// tools/sweep_timeline.py only (variant build): every workgroup of every sweep launch owns a slot of one stamp buffer (the stamps
// of the LAST iteration stay); meta: (tag, level, workgroups, KB, list, first slot) per launch
unsigned long long *g_swp_base; size_t g_swp_wgs; std::vector<int> g_swp_meta;
#endif
// ---- the sweeps -------------------------------------------------------------------------------------------------------------------
// The plan of both sweeps is a value that sweep_plan.hpp computes from the factor, the context's knobs and two numbers of the device:
// nothing here decides anything about it.  upload_factor: the limits, the plan, its ADMM_HIP_VERBOSE lines, (the profile build's
// slots,) the upload.

// ADMM_HIP_VERBOSE, the fused launches: one "plan fused" and one "plan fused_bwd" line per call (tests/test_sweep_subtree*.py assert
// the shapes they reach from them)
void print_fuse_plan(const admm_lib::FusePlan &P, int lds_cap) {
    if (P.why_off) fprintf(stderr, "admm_hip: plan fused off (%s)\n", P.why_off);
    else fprintf(stderr, "admm_hip: plan fused cut %d subtrees %d left %d lds %d cap %d levels %d..%d maxin %d skip %d empty %d\n", P.cut, P.n_fuse(), P.left, P.lds, lds_cap,
                 P.lv_min, P.lv_max, P.maxin, P.skip, P.empty);
    if (P.why_bwd_off) fprintf(stderr, "admm_hip: plan fused_bwd off (%s)\n", P.why_bwd_off);
    else fprintf(stderr, "admm_hip: plan fused_bwd cut %d subtrees %d left %d lds %d cap %d\n", P.cut, P.n_fuse_bwd(), P.candidates - P.n_fuse_bwd(), P.bwd_lds, lds_cap);
}

// ... and one pass over the levels, a line per level and one per root (tests/test_wide_supernodes.py asserts from them which kernel
// paths a scene reaches): column chunks of the widest block item, row chunks of the tallest front in the backward kernel, and per root
// its product's chunks
void print_level_plans(const admm_hip_ctx *ctx, const char *pass, const std::vector<admm_lib::LevelPlan> &levels) {
    using namespace admm_dev;
    for (size_t l = 0; l < levels.size(); ++l) {
        const admm_lib::LevelPlan &L = levels[l];
        const int kchunk = L.big_nw == 16 ? FwdBig<16>::KCHUNK : (L.big_nw == 8 ? FwdBig<8>::KCHUNK : FwdBig<4>::KCHUNK);
        int kmax = 0, fmax = 0;
        for (const SweepItem &q : L.big) kmax = std::max(kmax, q.k);
        for (const SweepItem &q : L.bwd) fmax = std::max(fmax, q.k + q.r);
        fprintf(stderr, "admm_hip: plan %s level %zu: fwd wave %d block %d big_nw %d kmax %d chunks %d | bwd cw %d nw %d items %d fmax %d rchunks %d | cg4 %d\n",
                pass, l, (int)L.small.size(), (int)L.big.size(), L.big_nw, kmax, (kmax + kchunk - 1) / kchunk, L.bwd_cw, L.bwd_nw, (int)L.bwd.size(), fmax,
                (fmax + BWD_RCHUNK - 1) / BWD_RCHUNK, ctx->F.cg4.empty() ? 0 : 1);
        for (const admm_lib::SweepRoot &R : L.roots)
            fprintf(stderr, "admm_hip: plan %s level %zu: root k %d %s chunks %d\n", pass, l, R.k, R.k <= ctx->root_fuse_k ? "fused" : "gather", (R.k + ROOT_KCHUNK - 1) / ROOT_KCHUNK);
    }
}

#ifdef ADMM_SWEEP_PROFILE
// the profile build's slots: every workgroup of every launch of the pass gets one, written into its items before they are uploaded
void profile_level_plans(std::vector<admm_lib::LevelPlan> &levels, int list) {
    for (size_t l = 0; l < levels.size(); ++l) {
        admm_lib::LevelPlan &L = levels[l];
        auto reg = [&](std::vector<admm_dev::SweepItem> &v, int group, int tag) {
            if (v.empty()) return;
            const int n_wg = ((int)v.size() + group - 1) / group;
            for (size_t i = 0; i < v.size(); ++i) v[i].pad2 = (v[i].k || v[i].r) ? (long long)(g_swp_wgs + i / group) : -1;
            for (int q : {tag, (int)l, n_wg, (int)(L.mbytes * 1024), list, (int)g_swp_wgs}) g_swp_meta.push_back(q);
            g_swp_wgs += n_wg;
        };
        reg(L.small, admm_dev::FWD_SMALL_WAVES, 0); reg(L.big, 1, L.big_nw); reg(L.bwd, 1, 100 + 10 * L.bwd_cw + (L.bwd_nw == 16 ? 6 : L.bwd_nw));
    }
}
#endif

int upload_level_plans(admm_hip_ctx *ctx, const std::vector<admm_lib::LevelPlan> &plans, std::vector<LevelDev> &into) {
    into.assign(plans.size(), LevelDev());
    for (size_t l = 0; l < plans.size(); ++l) {
        const admm_lib::LevelPlan &P = plans[l];
        LevelDev &L = into[l];
        L.level = (int)l; L.mbytes = P.mbytes; L.roots = P.roots;
        L.n_small = (int)P.small.size(); L.n_big = (int)P.big.size(); L.n_bwd = (int)P.bwd.size();
        L.big_nw = P.big_nw; L.bwd_cw = P.bwd_cw; L.bwd_nw = P.bwd_nw;
        TRY(upload(ctx, &L.d_small, P.small)); TRY(upload(ctx, &L.d_big, P.big)); TRY(upload(ctx, &L.d_bwd, P.bwd));
    }
    return ADMM_OK;
}

int upload_factor(admm_hip_ctx *ctx) {
    Factor &F = ctx->F;
    const int ns = (int)F.sn.size();
    const bool verbose = getenv("ADMM_HIP_VERBOSE") != nullptr;
    std::vector<int> first(ns), ncols(ns), nrows(ns);
    std::vector<int64_t> poff(ns), roff(ns), soff(ns), foff(ns);
    for (int s = 0; s < ns; ++s) { first[s] = F.sn[s].first; ncols[s] = F.sn[s].ncols; nrows[s] = F.sn[s].nrows; poff[s] = ctx->dev_panel_off[s]; roff[s] = F.sn[s].rows_off; soff[s] = F.sn[s].slot_off; foff[s] = F.sn[s].front_off; }
    TRY(dalloc(ctx, &ctx->d_panels, (size_t)std::max<int64_t>(ctx->dev_panels_size, 1)));      // (rank-local factorization: this rank's subtrees + the top only)
    TRY(panels_to_device(ctx));
    TRY(upload(ctx, &ctx->d_sn_first, first)); TRY(upload(ctx, &ctx->d_sn_ncols, ncols)); TRY(upload(ctx, &ctx->d_sn_nrows, nrows));
    TRY(upload(ctx, &ctx->d_sn_panel_off, poff)); TRY(upload(ctx, &ctx->d_sn_rows_off, roff)); TRY(upload(ctx, &ctx->d_sn_slot_off, soff));
    TRY(upload(ctx, &ctx->d_rows, F.rows));
    TRY(upload(ctx, &ctx->d_sn_front_off, foff));
    TRY(upload(ctx, &ctx->d_cg_ptr, F.cg_ptr)); TRY(upload(ctx, &ctx->d_cg_slot, F.cg_slot));
    ctx->d_cg4 = nullptr;
    if (!F.cg4.empty()) TRY(upload(ctx, &ctx->d_cg4, F.cg4));
    TRY(dalloc(ctx, &ctx->d_c, 3 * (size_t)std::max<int64_t>(F.n_slots, 1)));
    ctx->d_ainv = nullptr;
    if (ctx->dense) TRY(upload(ctx, &ctx->d_ainv, ctx->Ainv));

    // (1) the limits: a fused subtree's workgroup may take the LDS that leaves room for a second one on its CU
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ctx->device_id));
    const admm_lib::DeviceLimits limits{std::max(prop.multiProcessorCount, 1), (int)std::min<size_t>(prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor / 2)};

    // (2) the plan.  Plain: one pass over all supernodes.  Subtree sharding: this rank's own subtrees (the fused launches are among
    // them), then the replicated top, whose backward sweep only has to reach the separators this rank needs (partition.cpp: top_needs)
    const bool subtree = ctx->shard_mode == 1 && ctx->world > 1;
    const std::vector<int> *own = subtree ? &ctx->sn_owner : nullptr;
    const int want = subtree ? ctx->rank : 0;
    const admm_lib::FusePlan fuse = admm_lib::plan_fused_subtrees(F, ctx->dev_panel_off, ctx->dev_panels_size, own, want, ctx->knobs, limits);
    if (!fuse.error.empty()) return fail(ctx, ADMM_ERR_STATE, "%s", fuse.error.c_str());
    std::vector<char> top_needed;                 // this rank's
    std::vector<int> top_provider;
    if (subtree) {
        std::vector<std::vector<char> > need;
        top_needs(ctx, need, top_provider);
        top_needed = need[ctx->rank];
    }
    std::vector<admm_lib::LevelPlan> own_levels = admm_lib::plan_levels(F, ctx->dev_panel_off, ctx->dev_root_inv_off, own, want, top_needed, fuse.fused, fuse.fused_bwd, ctx->knobs), top_levels;
    if (subtree) top_levels = admm_lib::plan_levels(F, ctx->dev_panel_off, ctx->dev_root_inv_off, own, -1, top_needed, fuse.fused, fuse.fused_bwd, ctx->knobs);

    // (3) ADMM_HIP_VERBOSE
    if (verbose) {
        print_fuse_plan(fuse, limits.lds_cap);
        if (subtree) {
            int nt = 0, nn = 0;
            for (int s2 = 0; s2 < ns; ++s2) if (ctx->sn_owner[s2] < 0) { ++nt; nn += top_needed[s2] ? 1 : 0; }
            fprintf(stderr, "admm_hip: rank %d: backward sweep over %d of the %d top supernodes\n", ctx->rank, nn, nt);
        }
        print_level_plans(ctx, "own", own_levels); print_level_plans(ctx, "top", top_levels);
        if (subtree && ctx->dist_top)      // (the top's per-level lines above are not run: the root's rows are this rank's product)
            fprintf(stderr, "admm_hip: plan dist-top rank %d: root k %d rows %d..%d nrows %d chunks %d\n", ctx->rank, ctx->root_k, ctx->root_r0, ctx->root_r1,
                    ctx->root_r1 - ctx->root_r0, (ctx->root_k + admm_dev::ROOT_KCHUNK - 1) / admm_dev::ROOT_KCHUNK);
    }
#ifdef ADMM_SWEEP_PROFILE
    {
        g_swp_wgs = 0; g_swp_meta.clear();
        profile_level_plans(own_levels, 0); profile_level_plans(top_levels, 100);
        unsigned long long *p = nullptr;
        TRY(dalloc(ctx, (double **)&p, 4 * g_swp_wgs + 4));
        HIPCHK(hipMemset(p, 0, sizeof(unsigned long long) * (4 * g_swp_wgs + 4)));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(admm_dev::g_sweep_prof), &p, sizeof(p)));
        g_swp_base = p;
    }
#endif

    // (4) the upload
    ctx->fuse_cut = fuse.n_fuse() ? fuse.cut : -1; ctx->n_fuse = fuse.n_fuse(); ctx->fuse_lds = fuse.lds;
    ctx->n_fuse_bwd = fuse.n_fuse_bwd(); ctx->fuse_bwd_lds = fuse.bwd_lds;
    if (fuse.n_fuse()) { TRY(upload(ctx, &ctx->d_fuse_rec, fuse.rec)); TRY(upload(ctx, &ctx->d_fuse_off, fuse.off)); }
    if (fuse.n_fuse_bwd()) { TRY(upload(ctx, &ctx->d_fuse_bwd_rec, fuse.bwd_rec)); TRY(upload(ctx, &ctx->d_fuse_bwd_off, fuse.bwd_off)); }
    TRY(upload_level_plans(ctx, own_levels, ctx->levels)); TRY(upload_level_plans(ctx, top_levels, ctx->levels_top));
    ctx->n_comm_top = ctx->n_comm_slots = 0;
    ctx->d_comm_top = ctx->d_comm_slots = nullptr; ctx->d_comm_mine = ctx->d_base_mask = ctx->d_keep_mask = nullptr; ctx->d_comm_buf = nullptr;
    if (subtree) {      // the exchange lists (see shard_pack_kernel) and the node masks
        const admm_lib::ShardExchange E = admm_lib::plan_shard_exchange(F, ctx->sn_owner, ctx->node_owner, top_provider, ctx->rank);
        ctx->n_comm_top = (int)E.top_nodes.size(); ctx->n_comm_slots = (int)E.slots.size();
        TRY(upload(ctx, &ctx->d_comm_top, E.top_nodes)); TRY(upload(ctx, &ctx->d_comm_slots, E.slots)); TRY(upload(ctx, &ctx->d_comm_mine, E.mine));
        TRY(upload(ctx, &ctx->d_base_mask, E.base)); TRY(upload(ctx, &ctx->d_keep_mask, E.keep));
        TRY(dalloc(ctx, &ctx->d_comm_buf, 3 * (size_t)std::max(1, ctx->n_comm_top + ctx->n_comm_slots)));
    }
    return ADMM_OK;
}

// the scale s of an element's energy (energy.hpp): the rest measure of the hyperelastic kinds, stiffness * measure of the blended tets
// and triangles (the local step's kblend), the stiffness of springs and hinges, weight^2 of an anchor (the anchor kernel reads the live
// weight^2 instead, which admm_hip_recompute_weights refreshes); 0 for what is not evaluated
double energy_scale(const Batch &b, int e) {
    const int np = b.kind < ADMM_KIND_COUNT ? ADMM_KIND_PARAMS[b.kind] : 0;
    switch (b.kind) {
    case ADMM_KIND_TET_NH: case ADMM_KIND_TET_STVK: case ADMM_KIND_TRI_FUNG: return b.measure[e];
    case ADMM_KIND_TET_LINEAR: case ADMM_KIND_TET_VOLUME: case ADMM_KIND_TRI_STRAIN: case ADMM_KIND_TRI_AREA: return b.params[(size_t)e * np] * b.measure[e];
    case ADMM_KIND_SPRING: case ADMM_KIND_BEND: return b.params[(size_t)e * np];
    case ADMM_KIND_ANCHOR: return b.weight[e] * b.weight[e];
    }
    return 0.0;
}

// the moving friction kernel's table (kernels_collision.hpp), one entry per mesh: its corner ids, its vertex velocities (null: none in
// effect), a body surface's coefficient and flag.  Written at finalize and again by every call that changes what moves (abi_setup.inc:
// push_shapes).  At finalize an obstacle has d_vel == nullptr and has_vel == false and a body surface's buffer has just been allocated,
// so the one formula gives what finalize needs too.
std::vector<admm_mesh::MeshMotion> mesh_motion_table(const admm_hip_ctx *ctx) {
    std::vector<admm_mesh::MeshMotion> mo(ctx->meshes.size());
    for (size_t mi = 0; mi < mo.size(); ++mi) {
        const admm_hip_ctx::CollisionMesh &m = ctx->meshes[mi];
        const bool body = m.body();
        mo[mi] = admm_mesh::MeshMotion{m.upd.cid, (body || m.has_vel) ? m.d_vel : nullptr, body ? m.body_mu : 0.0, body ? 1 : 0, 0};
    }
    return mo;
}

// the records' part in the device tables, planned on the host (collision_plan.hpp); finalize, once F.iperm stands
admm_lib::MeshTables plan_context_meshes(const admm_hip_ctx *ctx) {
    std::vector<admm_lib::MeshPlanInput> in;
    for (const admm_hip_ctx::CollisionMesh &m : ctx->meshes)
        in.push_back(admm_lib::MeshPlanInput{m.own_first, m.own_count, m.body_nodes.data(), (int)m.body_nodes.size(), m.self_collision,
                                             {m.body_self[0], m.body_self[1], m.body_self[2]}, m.side_reach});
    return admm_lib::plan_mesh_tables(ctx->n_nodes, ctx->F.iperm.data(), in);
}

// mesh obstacles and surfaces: every mesh's BVH nodes, triangles and pseudo-normals, the table of them the kernels read (d_meshes) and
// the per-feature tables parallel to it.  A table of the plan that is empty is not uploaded and its pointer stays null, so that a
// context without the feature holds and launches what it did (launch.inc: collision_tables).
int upload_meshes(admm_hip_ctx *ctx, const admm_lib::MeshTables &plan) {
    const int n = ctx->n_nodes;
    const size_t nm = ctx->meshes.size();
    ctx->d_body_tag = nullptr; ctx->d_mesh_self = nullptr; ctx->d_self_vid = nullptr; ctx->d_mesh_bself = nullptr; ctx->d_mesh_rest = nullptr;
    ctx->d_mesh_reach = nullptr; ctx->d_mesh_side_slot = nullptr; ctx->d_mesh_bnd = nullptr; ctx->d_side = nullptr;
    if (!plan.tag.empty()) TRY(upload(ctx, &ctx->d_body_tag, plan.tag));
    if (plan.any_sheet_self) TRY(upload(ctx, &ctx->d_mesh_self, plan.self_flag));
    if (plan.any_sheet_self || plan.any_body_self) TRY(upload(ctx, &ctx->d_self_vid, plan.vid));
    if (plan.any_body_self) {      // ... with the rest vertices of the body surfaces that collide with themselves
        std::vector<const double *> rest(nm, nullptr);
        for (size_t mi = 0; mi < nm; ++mi) {
            if (!(ctx->meshes[mi].body_self[0] > 0.0)) continue;
            double *rv = nullptr;
            TRY(upload(ctx, &rv, ctx->meshes[mi].rest));
            rest[mi] = rv;
        }
        TRY(upload(ctx, &ctx->d_mesh_bself, plan.body_self)); TRY(upload(ctx, &ctx->d_mesh_rest, rest));
    }
    std::vector<admm_mesh::MeshDev> md;
    std::vector<double> thick(nm);
    for (size_t mi = 0; mi < nm; ++mi) {
        admm_hip_ctx::CollisionMesh &m = ctx->meshes[mi];
        const admm_hip_mesh &M = m.mesh;
        admm_mesh::MeshDev d{};
        d.owner = plan.owner[mi];
        admm_mesh::Node *nd; admm_mesh::Tri *tr; admm_mesh::Nrm *nr;
        TRY(upload(ctx, &nd, M.nodes)); TRY(upload(ctx, &tr, M.tris)); TRY(upload(ctx, &nr, M.nrm));
        d.nodes = nd; d.tris = tr; d.nrm = nr; d.n_nodes = (int)M.nodes.size(); d.n_tris = (int)M.tris.size();
        md.push_back(d);
        thick[mi] = M.thickness;
        // what admm_hip_update_collision_mesh needs (kernels_mesh.hpp): neither it nor step allocates
        admm_hip_ctx::MeshUpdate u{};
        u.nodes = nd; u.tris = tr; u.nrm = nr;
        const size_t nt = M.tris.size();
        TRY(dalloc(ctx, &u.verts, 3 * (size_t)M.nv)); TRY(dalloc(ctx, &u.fn, 3 * nt)); TRY(dalloc(ctx, &u.vn, 3 * (size_t)M.nv));
        TRY(dalloc(ctx, &u.part, (nt + admm_mesh::VOL_CHUNK - 1) / admm_mesh::VOL_CHUNK));
        TRY(upload(ctx, &u.cid, M.cid)); TRY(upload(ctx, &u.adj, M.adj)); TRY(upload(ctx, &u.inc_ptr, M.inc_ptr)); TRY(upload(ctx, &u.inc, M.inc));
        TRY(upload(ctx, &u.lvl_nodes, M.lvl_nodes));
        // the moving friction kernel's velocities: an obstacle's buffer is allocated by admm_hip_set_collision_mesh_velocity
        m.d_vel = nullptr; m.has_vel = false;
        if (m.body()) {      // a body surface: its vertices' device node ids, its own check (re-armed by the device) and status, and its velocity buffer, which lives from here on (zero: v at finalize)
            std::vector<int> dn(m.body_nodes.size());
            for (size_t k = 0; k < dn.size(); ++k) dn[k] = ctx->F.iperm[m.body_nodes[k]];
            TRY(upload(ctx, &u.dnode, dn));
            TRY(upload(ctx, &u.chk, std::vector<admm_mesh::UpdateCheck>(1, admm_mesh::UpdateCheck{admm_mesh::NO_TRI, admm_mesh::NO_TRI, 0.0})));
            TRY(upload(ctx, &u.status, std::vector<admm_mesh::BodyStatus>(1, admm_mesh::BodyStatus{0, 0, -1, 0})));
            TRY(dalloc(ctx, &m.d_vel, 3 * (size_t)M.nv));
            HIPCHK(hipMemset(m.d_vel, 0, sizeof(double) * 3 * (size_t)M.nv));
        }
        m.upd = u;
    }
    TRY(upload(ctx, &ctx->d_mesh_motion, mesh_motion_table(ctx)));
    TRY(upload(ctx, &ctx->d_mesh_thick, thick));
    TRY(upload(ctx, &ctx->d_meshes, md));
    TRY(dalloc(ctx, &ctx->d_mesh_chk, 1));
    if (plan.n_side_rows > 0) {      // side memory: the reach, the row of sides and the boundary table of every mesh, and the sides themselves (zero)
        std::vector<double> reach(nm, 0.0);
        std::vector<const int *> bnd(nm, nullptr);
        for (size_t mi = 0; mi < nm; ++mi) {
            if (plan.side_row[mi] < 0) continue;
            reach[mi] = ctx->meshes[mi].side_reach;
            int *b = nullptr;
            TRY(upload(ctx, &b, ctx->meshes[mi].mesh.bnd));
            bnd[mi] = b;
        }
        TRY(upload(ctx, &ctx->d_mesh_reach, reach)); TRY(upload(ctx, &ctx->d_mesh_side_slot, plan.side_row)); TRY(upload(ctx, &ctx->d_mesh_bnd, bnd));
        TRY(dalloc(ctx, &ctx->d_side, (size_t)plan.n_side_rows * (size_t)n));
        HIPCHK(hipMemset(ctx->d_side, 0, sizeof(int32_t) * (size_t)plan.n_side_rows * (size_t)n));
    }
    return ADMM_OK;
}

int upload_all(admm_hip_ctx *ctx, const admm_lib::MeshTables &plan) {
    const double t0 = now_s();
    const int n = ctx->n_nodes;
    const Factor &F = ctx->F;
    HIPCHK(hipSetDevice(ctx->device_id));
    free_device(ctx);
    ctx->res_ready = false;
    // (Anderson acceleration's buffers went with the rest: the next accelerated step creates them again)
    ctx->d_aa_seg = nullptr; ctx->d_aa_state = nullptr; ctx->d_aa_log = nullptr; ctx->d_aa_sin = nullptr; ctx->d_aa_ring = nullptr; ctx->d_aa_part = nullptr;
    ctx->aa_cap_m = 0; ctx->aa_log_cap = 0; ctx->aa_log_n = 0; ctx->aa_ran = false;
    for (Batch &b : ctx->batches) b.d_G = nullptr;
    {
        std::vector<double> px = permute_nodes(ctx->x, F.perm, 3), pv = permute_nodes(ctx->v, F.perm, 3), pm = permute_nodes(ctx->m3, F.perm, 3);
        TRY(upload(ctx, &ctx->d_x, px)); TRY(upload(ctx, &ctx->d_v, pv)); TRY(upload(ctx, &ctx->d_m3, pm));
        TRY(upload(ctx, &ctx->d_xcur, px));
        TRY(dalloc(ctx, &ctx->d_mxbar, 3 * (size_t)n)); TRY(dalloc(ctx, &ctx->d_y, 3 * (size_t)n)); TRY(dalloc(ctx, &ctx->d_w, 3 * (size_t)n));
        TRY(upload(ctx, &ctx->d_perm, F.perm)); TRY(dalloc(ctx, &ctx->d_stage, 6 * (size_t)n));
        TRY(upload(ctx, &ctx->d_iperm, F.iperm));
    }
    TRY(upload_factor(ctx));
    // batches: shard, sort corners, SoA upload
    int64_t slot = 0, nloc = 0;
    // pass 1: local ranges, corner order, incidence counts per (factor-order) node
    std::vector<int64_t> inc_ptr(n + 1, 0);
    for (Batch &b : ctx->batches) {
        if (b.kind == ADMM_KIND_GENERIC) {      // one slot per (element, node)
            b.slot_base = slot;
            for (int el = 0; el < b.n_local; ++el) {
                const int32_t *nd; const int nn = b.elem_nodes(b.local[el], &nd);
                for (int c = 0; c < nn; ++c) inc_ptr[F.iperm[nd[c]] + 1]++;
                slot += nn;
            }
            nloc += b.n_local;
            continue;
        }
        const int nn = ADMM_KIND_NODES[b.kind];
        b.slot_base = slot;
        const bool is_tri = b.kind == ADMM_KIND_TRI_STRAIN || b.kind == ADMM_KIND_TRI_AREA || b.kind == ADMM_KIND_TRI_FUNG;
        const bool sort_corners = (b.kind >= ADMM_KIND_TET_LINEAR && b.kind <= ADMM_KIND_TET_STVK) || is_tri;
        b.max_iter = 0;
        if (b.kind == ADMM_KIND_TET_NH || b.kind == ADMM_KIND_TET_STVK)
            for (int e = 0; e < b.n_total; ++e) b.max_iter = std::max(b.max_iter, (int)b.params[(size_t)e * 3 + 2]);
        b.corner_perm.assign((size_t)b.n_total * nn, 0);
        b.prered = ctx->tet_prered && b.kind >= ADMM_KIND_TET_LINEAR && b.kind <= ADMM_KIND_TET_STVK;
        b.tpb = admm_dev::LOCAL_BLOCK;
        if (b.kind == ADMM_KIND_TET_NH || b.kind == ADMM_KIND_TET_STVK) {
            // Fewer tets per one-wave block (the lanes beyond idle) shortens the union of paths a wave executes.  Measured (profiles/r04/underfilled.txt):
            // it pays only where the launch is under-filled AND ends in a long tail of a few pathological tets -- BASELINE configs[2] (50 700 StVK tets)
            // at frame 14: local step 136 -> 126 us (32 per block) -> 120 us (16); the same bar at frame 8: 78 -> 76 -> 92 us; Neo-Hookean bars of
            // 5 400 / 18 000 / 50 700 / 125 000 tets: 42 -> 47, 69 -> 72, 73 -> 75, 84 -> 98 us with 32 per block.  No size rule separates the cases
            // (the tail comes and goes with the deformation), so the default stays 64; ADMM_HIP_TPB sets it by hand.
            if (ctx->tet_tpb > 0) b.tpb = ctx->tet_tpb;
        }
        std::vector<int> blk_nodes;       // prered: the nodes of the current 64-tet block
        for (int el = 0; el < b.n_local; ++el) {
            const int e = b.local[el];
            const int *id = b.idx.data() + (size_t)e * nn;
            int ord[4] = {0, 1, 2, 3};
            if (sort_corners) std::stable_sort(ord, ord + nn, [&](int a, int c) { return id[a] < id[c]; });
            for (int c = 0; c < nn; ++c) {
                b.corner_perm[(size_t)e * nn + c] = ord[c];
                if (b.prered) blk_nodes.push_back(F.iperm[id[ord[c]]]); else inc_ptr[F.iperm[id[ord[c]]] + 1]++;
            }
            if (b.prered && (block_end(b, el) || el + 1 == b.n_local)) {      // one slot per distinct node of the block
                std::sort(blk_nodes.begin(), blk_nodes.end());
                blk_nodes.erase(std::unique(blk_nodes.begin(), blk_nodes.end()), blk_nodes.end());
                for (int pn : blk_nodes) inc_ptr[pn + 1]++;
                slot += (int64_t)blk_nodes.size();
                blk_nodes.clear();
            }
        }
        if (!b.prered) slot += (int64_t)b.n_local * nn;
        nloc += b.n_local;
    }
    int64_t maxdeg = 0;
    for (int i = 0; i < n; ++i) { maxdeg = std::max(maxdeg, inc_ptr[i + 1]); inc_ptr[i + 1] += inc_ptr[i]; }
    std::vector<int64_t> inc_pos(inc_ptr.begin(), inc_ptr.end() - 1);
    // RHS slot layout.  Node-sorted (a node's incidences contiguous) makes the gather's lanes -- one per (node, component) --
    // read 24-byte pieces 0.5 KB apart; rank-major (all nodes' r-th incidence contiguous) makes neighbouring lanes read
    // neighbouring words for every r, and neighbouring tets of a wave write neighbouring slots.  Same summation order per node
    // (r ascending = batch, element, corner), so the results are bitwise the same.  It pads every node to the largest incidence
    // count: used unless that more than doubles the array (meshes with a few very high-valence nodes).
    ctx->slot_stride = (maxdeg * n <= 2 * inc_ptr[n] + 1024 && getenv("ADMM_HIP_SLOTS_NODE_SORTED") == nullptr) ? n : 0;
    if (getenv("ADMM_HIP_VERBOSE"))      // the layout this context's right-hand side is assembled in (tests/test_rhs_reference.py asserts it)
        fprintf(stderr, "admm_hip: plan rhs: slots %lld maxdeg %lld layout %s prered %d\n", (long long)inc_ptr[n], (long long)maxdeg,
                ctx->slot_stride ? "rank-major" : "node-sorted", ctx->tet_prered ? 1 : 0);
    // pass 2: device arrays; every corner gets the next slot of its node (fixed order: batch, element, corner)
    for (Batch &b : ctx->batches) {
        if (b.kind == ADMM_KIND_GENERIC) {
            // this rank's rows (CSR in factor-order dofs) and, per (element, node) slot and component, the rows that feed it
            std::vector<int> lrow, rptr(1, 0), col, sptr(1, 0), srow, sdst;
            std::vector<double> val;
            b.g_sval.clear(); b.g_srow_b.clear();
            for (int el = 0; el < b.n_local; ++el) {
                const int e = b.local[el];
                const int32_t *nd; const int nn = b.elem_nodes(e, &nd);
                for (int64_t r = b.g_elem_row[e]; r < b.g_elem_row[e + 1]; ++r) {
                    lrow.push_back((int)(b.g_row0 + r));
                    for (int64_t p = b.g_rowptr[r]; p < b.g_rowptr[r + 1]; ++p) { col.push_back(3 * F.iperm[b.g_col[p] / 3] + b.g_col[p] % 3); val.push_back(b.g_val[p]); }
                    rptr.push_back((int)col.size());
                }
                // the element's entries by column (ascending row inside a column): one pass, an element may span all nodes
                std::vector<std::pair<int32_t, int64_t> > bycol;      // (column, entry)
                for (int64_t rr = b.g_elem_row[e]; rr < b.g_elem_row[e + 1]; ++rr) for (int64_t p = b.g_rowptr[rr]; p < b.g_rowptr[rr + 1]; ++p) bycol.push_back({b.g_col[p], p});
                std::stable_sort(bycol.begin(), bycol.end(), [](const std::pair<int32_t, int64_t> &x, const std::pair<int32_t, int64_t> &y) { return x.first < y.first; });
                std::vector<int64_t> entry_row(b.g_rowptr[b.g_elem_row[e + 1]] - b.g_rowptr[b.g_elem_row[e]]);
                for (int64_t rr = b.g_elem_row[e]; rr < b.g_elem_row[e + 1]; ++rr) for (int64_t p = b.g_rowptr[rr]; p < b.g_rowptr[rr + 1]; ++p) entry_row[p - b.g_rowptr[b.g_elem_row[e]]] = rr;
                size_t q = 0;
                for (int c = 0; c < nn; ++c) {
                    const int pn = F.iperm[nd[c]];
                    const int64_t r = inc_pos[pn]++;
                    sdst.push_back(ctx->slot_stride ? (int)((r - inc_ptr[pn]) * ctx->slot_stride + pn) : (int)r);
                    for (int comp = 0; comp < 3; ++comp) {
                        for (; q < bycol.size() && bycol[q].first == 3 * nd[c] + comp; ++q) {
                            const int64_t p = bycol[q].second, rr = entry_row[p - b.g_rowptr[b.g_elem_row[e]]];
                            srow.push_back((int)(b.g_row0 + rr)); b.g_srow_b.push_back((int32_t)rr); b.g_sval.push_back(b.g_val[p]);
                        }
                        sptr.push_back((int)srow.size());
                    }
                }
            }
            b.g_lrows = (int)lrow.size(); b.g_lslots = (int)sdst.size();
            std::vector<double> coef(b.g_sval.size());
            for (size_t i = 0; i < coef.size(); ++i) { const double w = b.g_roww[b.g_srow_b[i]]; coef[i] = b.g_sval[i] * ((ctx->dt * ctx->dt) * (w * w)); }
            TRY(upload(ctx, &b.d_g_lrow, lrow)); TRY(upload(ctx, &b.d_g_rptr, rptr)); TRY(upload(ctx, &b.d_g_col, col)); TRY(upload(ctx, &b.d_g_val, val));
            TRY(upload(ctx, &b.d_g_sptr, sptr)); TRY(upload(ctx, &b.d_g_srow, srow)); TRY(upload(ctx, &b.d_g_sdst, sdst)); TRY(upload(ctx, &b.d_g_scoef, coef));
            continue;
        }
        const int nn = ADMM_KIND_NODES[b.kind], np = ADMM_KIND_PARAMS[b.kind], rows = ADMM_KIND_ROWS[b.kind], ist = idx_stride(b.kind);
        const int nl = b.n_local;
        std::vector<int> idx((size_t)std::max(nl, 1) * ist, 0), dst((size_t)std::max(nl, 1) * ist, 0);
        b.G.assign((size_t)12 * std::max(nl, 1), 0.0);
        std::vector<double> rest((size_t)12 * std::max(nl, 1), 0.0), par((size_t)std::max(np, 1) * std::max(nl, 1), 0.0), w2h2(std::max(nl, 1)), kbl(std::max(nl, 1)), w2(std::max(nl, 1)), esc(std::max(nl, 1));
        // prered: per block, the corners sorted by (node, lane, corner) -> pos4 (where a corner's share goes in the block's LDS
        // staging, one byte per corner), and per distinct node an entry (slot, end of its run in the staging)
        std::vector<unsigned int> pos4(b.prered ? (size_t)std::max(nl, 1) : 0, 0u);
        std::vector<int> bn_ptr(1, 0), bn_dst; std::vector<unsigned short> bn_end;
        struct Corner { int pn; unsigned short lc; };      // lc = lane * 4 + corner
        std::vector<Corner> blk_c;
        int blk_first = 0;
        for (int el = 0; el < nl; ++el) {
            const int e = b.local[el];
            const int *id = b.idx.data() + (size_t)e * nn;
            const int *ord = b.corner_perm.data() + (size_t)e * nn;
            for (int c = 0; c < nn; ++c) {
                const int pn = F.iperm[id[ord[c]]];
                idx[(size_t)el * ist + c] = pn;
                if (b.prered) { blk_c.push_back({pn, (unsigned short)((el - blk_first) * 4 + c)}); continue; }
                const int64_t r = inc_pos[pn]++;
                dst[(size_t)el * ist + c] = ctx->slot_stride ? (int)((r - inc_ptr[pn]) * ctx->slot_stride + pn) : (int)r;
            }
            if (b.prered && (block_end(b, el) || el + 1 == nl)) {
                std::stable_sort(blk_c.begin(), blk_c.end(), [](const Corner &x, const Corner &y) { return x.pn < y.pn || (x.pn == y.pn && x.lc < y.lc); });
                for (size_t k = 0; k < blk_c.size(); ++k) {
                    const int lane = blk_c[k].lc >> 2, c = blk_c[k].lc & 3;
                    pos4[(size_t)blk_first + lane] |= (unsigned int)k << (8 * c);
                    if (k + 1 == blk_c.size() || blk_c[k + 1].pn != blk_c[k].pn) {
                        const int pn = blk_c[k].pn;
                        const int64_t r = inc_pos[pn]++;
                        bn_dst.push_back(ctx->slot_stride ? (int)((r - inc_ptr[pn]) * ctx->slot_stride + pn) : (int)r);
                        bn_end.push_back((unsigned short)(k + 1));
                    }
                }
                bn_ptr.push_back((int)bn_dst.size());
                blk_c.clear(); blk_first = el + 1;
            }
            const double *R = &b.rest[(size_t)e * 12];
            if (b.kind >= ADMM_KIND_TET_LINEAR && b.kind <= ADMM_KIND_TET_STVK) {
                for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) rest[(size_t)(c + 4 * r) * nl + el] = R[ord[c] + 4 * r];
            } else if (b.kind == ADMM_KIND_TRI_STRAIN || b.kind == ADMM_KIND_TRI_AREA || b.kind == ADMM_KIND_TRI_FUNG) {
                for (int c = 0; c < 3; ++c) for (int r = 0; r < 2; ++r) rest[(size_t)(c + 3 * r) * nl + el] = R[ord[c] + 3 * r];
            } else {
                for (int i = 0; i < 12; ++i) rest[(size_t)i * nl + el] = R[i];
            }
            {   // selector block in device corner order (residual tracking)
                double Gm[4][3]; int cols;
                element_G(b.kind, R, Gm, cols);
                for (int c = 0; c < nn; ++c) for (int r = 0; r < 3; ++r) b.G[(size_t)(3 * c + r) * nl + el] = Gm[ord[c]][r];
            }
            for (int p = 0; p < np; ++p) par[(size_t)p * nl + el] = b.params[(size_t)e * np + p];
            const double w = b.weight[e];
            w2[el] = w * w;
            w2h2[el] = (ctx->dt * ctx->dt) * (w * w);
            kbl[el] = b.params[(size_t)e * np] * b.measure[e];
            esc[el] = energy_scale(b, e);
        }
        b.d_pos4 = nullptr; b.d_bn_ptr = nullptr; b.d_bn_dst = nullptr; b.d_bn_end = nullptr;
        if (b.prered) { TRY(upload(ctx, &b.d_pos4, pos4)); TRY(upload(ctx, &b.d_bn_ptr, bn_ptr)); TRY(upload(ctx, &b.d_bn_dst, bn_dst)); TRY(upload(ctx, &b.d_bn_end, bn_end)); }
        TRY(upload(ctx, &b.d_idx, idx)); TRY(upload(ctx, &b.d_dst, dst)); TRY(upload(ctx, &b.d_rest, rest)); TRY(upload(ctx, &b.d_par, par));
        TRY(upload(ctx, &b.d_w2h2, w2h2)); TRY(upload(ctx, &b.d_kblend, kbl)); TRY(upload(ctx, &b.d_w2, w2));
        TRY(upload(ctx, &b.d_escale, esc));
        TRY(dalloc(ctx, &b.d_u, (size_t)rows * std::max(nl, 1))); TRY(dalloc(ctx, &b.d_z, (size_t)rows * std::max(nl, 1)));
        HIPCHK(hipMemset(b.d_u, 0, sizeof(double) * (size_t)rows * std::max(nl, 1)));
        HIPCHK(hipMemset(b.d_z, 0, sizeof(double) * (size_t)rows * std::max(nl, 1)));
        std::vector<double> st((size_t)4 * std::max(nl, 1), 1.0);
        TRY(upload(ctx, &b.d_state, st));
        TRY(dalloc(ctx, &b.d_niters, (size_t)std::max(nl, 1)));
        HIPCHK(hipMemset(b.d_niters, 0, sizeof(int) * (size_t)std::max(nl, 1)));
        b.d_order = nullptr; b.d_cost = nullptr; b.n_blocks_ordered = 0;
        {
            // more blocks than the chip holds at once (2 waves x 4 SIMDs x 256 CUs): the launch order matters
            const int nblk = batch_blocks(b);
            if ((b.kind == ADMM_KIND_TET_NH || b.kind == ADMM_KIND_TET_STVK) && ctx->tet_order && nblk > ctx->tet_order_min_blocks) {
                std::vector<int> ident(nblk); std::iota(ident.begin(), ident.end(), 0);
                TRY(upload(ctx, &b.d_order, ident));
                TRY(dalloc(ctx, &b.d_cost, (size_t)nblk));
                HIPCHK(hipMemset(b.d_cost, 0, sizeof(unsigned int) * (size_t)nblk));
                b.n_blocks_ordered = nblk;
            }
        }
        if (b.kind == ADMM_KIND_ANCHOR) {
            std::vector<double> tg((size_t)3 * std::max(nl, 1), 0.0); std::vector<int> ac(std::max(nl, 1), 1);
            for (int el = 0; el < nl; ++el) { for (int j = 0; j < 3; ++j) tg[3 * (size_t)el + j] = b.targets[3 * (size_t)b.local[el] + j]; ac[el] = b.active[b.local[el]]; }
            TRY(upload(ctx, &b.d_targets, tg)); TRY(upload(ctx, &b.d_active, ac));
        }
    }
    ctx->info.n_elems_local = nloc;
    ctx->info.rhs_slots = slot;
    if (ctx->slot_stride) slot = maxdeg * n;
    if (slot >= (int64_t)1 << 31) return fail(ctx, ADMM_ERR_UNSUPPORTED, "more than 2^31 RHS slots");
    ctx->n_fslots = slot;
    TRY(dalloc(ctx, &ctx->d_fslot, 3 * (size_t)std::max<int64_t>(slot, 1)));
    HIPCHK(hipMemset(ctx->d_fslot, 0, sizeof(double) * 3 * (size_t)std::max<int64_t>(slot, 1)));
    TRY(upload(ctx, &ctx->d_inc_ptr, inc_ptr));
    if (ctx->n_gen_rows) {      // user-defined forces: device and pinned host images of the generic row space
        const size_t bytes = sizeof(double) * (size_t)ctx->n_gen_rows;
        TRY(dalloc(ctx, &ctx->d_gen_dx, (size_t)ctx->n_gen_rows)); TRY(dalloc(ctx, &ctx->d_gen_q, (size_t)ctx->n_gen_rows));
        HIPCHK(hipMemset(ctx->d_gen_dx, 0, bytes)); HIPCHK(hipMemset(ctx->d_gen_q, 0, bytes));
        if (!ctx->h_gen_dx) {
            HIPCHK(hipHostMalloc((void **)&ctx->h_gen_dx, bytes)); HIPCHK(hipHostMalloc((void **)&ctx->h_gen_u, bytes));
            HIPCHK(hipHostMalloc((void **)&ctx->h_gen_z, bytes)); HIPCHK(hipHostMalloc((void **)&ctx->h_gen_q, bytes));
            HIPCHK(hipEventCreateWithFlags(&ctx->gen_ev, hipEventDisableTiming));
        }
        std::memset(ctx->h_gen_dx, 0, bytes); std::memset(ctx->h_gen_u, 0, bytes); std::memset(ctx->h_gen_z, 0, bytes); std::memset(ctx->h_gen_q, 0, bytes);
    }
    // collision shapes and the general explicit forces (index lists in factor order)
    TRY(dalloc(ctx, &ctx->d_shapes, 1));
    HIPCHK(hipMemcpy(ctx->d_shapes, &ctx->shapes, sizeof(admm_dev::ShapeTable), hipMemcpyHostToDevice));
    if (!ctx->meshes.empty()) TRY(upload_meshes(ctx, plan));
    for (Explicit &E : ctx->explicits) {
        std::vector<int> pidx(E.idx.size());
        for (size_t i = 0; i < E.idx.size(); ++i) pidx[i] = F.iperm[E.idx[i]];
        E.d_idx = nullptr;
        if (E.type == ADMM_EXPLICIT_WIND && E.n) {
            // dependency levels of the serial loop: level(t) = 1 + max level of earlier triangles sharing a node
            std::vector<int> last(n, 0), lev(E.n);
            int nlev = 0;
            for (int t = 0; t < E.n; ++t) {
                const int *q = &pidx[3 * (size_t)t];
                const int l = 1 + std::max(last[q[0]], std::max(last[q[1]], last[q[2]]));
                lev[t] = l; last[q[0]] = last[q[1]] = last[q[2]] = l; nlev = std::max(nlev, l);
            }
            std::vector<int> lptr(nlev + 1, 0);
            for (int t = 0; t < E.n; ++t) lptr[lev[t]]++;            // level l (1-based) counted into lptr[l]
            for (int l = 0; l < nlev; ++l) lptr[l + 1] += lptr[l];   // lptr[l] = end of level l = start of level l+1
            std::vector<int> pos(lptr.begin(), lptr.end() - 1), sorted(pidx.size());
            for (int t = 0; t < E.n; ++t) { const int d = pos[lev[t] - 1]++; for (int c = 0; c < 3; ++c) sorted[3 * (size_t)d + c] = pidx[3 * (size_t)t + c]; }
            E.n_levels = nlev;
            TRY(upload(ctx, &E.d_idx, sorted)); TRY(upload(ctx, &E.d_level_ptr, lptr));
        } else if (!pidx.empty()) TRY(upload(ctx, &E.d_idx, pidx));
    }
    // damping groups (kernels_damping.hpp): one block per 64 consecutive nodes of a group, counted from its first node; a context with
    // no group uploads nothing
    ctx->damp_blocks = 0; ctx->d_damp_blk = ctx->d_damp_grp = ctx->d_damp_rate = ctx->d_damp_mom = nullptr; ctx->d_damp_vc = ctx->d_damp_part = nullptr;
    if (!ctx->damp_groups.empty()) {
        using namespace admm_dev;
        const size_t ng = ctx->damp_groups.size();
        std::vector<DampGroup> grp(ng); std::vector<DampBlock> blk;
        for (size_t g = 0; g < ng; ++g) {
            admm_hip_ctx::DampGroupHost &H = ctx->damp_groups[g];
            const int nb = (H.node_count + DAMP_BLOCK - 1) / DAMP_BLOCK;
            grp[g] = DampGroup{H.node_first, H.node_count, (int)blk.size(), nb};
            for (int b = 0; b < nb; ++b) blk.push_back(DampBlock{(int)g, H.node_first + b * DAMP_BLOCK});
            H.rate_dirty = true;
        }
        ctx->damp_blocks = (int)blk.size();
        DampBlock *db = nullptr; DampGroup *dg = nullptr; DampRate *dr = nullptr; admm_damping::Moments *dm = nullptr;
        TRY(upload(ctx, &db, blk)); TRY(upload(ctx, &dg, grp)); TRY(dalloc(ctx, &dr, ng)); TRY(dalloc(ctx, &dm, ng));
        TRY(dalloc(ctx, &ctx->d_damp_vc, 3 * ng)); TRY(dalloc(ctx, &ctx->d_damp_part, (size_t)admm_damping::N_SUMS_2 * blk.size()));
        HIPCHK(hipMemset(dr, 0, sizeof(DampRate) * ng)); HIPCHK(hipMemset(dm, 0, sizeof(admm_damping::Moments) * ng)); HIPCHK(hipMemset(ctx->d_damp_vc, 0, sizeof(double) * 3 * ng));
        ctx->d_damp_blk = db; ctx->d_damp_grp = dg; ctx->d_damp_rate = dr; ctx->d_damp_mom = dm;
    }
    // pressure chambers (kernels_pressure.hpp): one block per 64 consecutive triangles of a chamber, counted from its first; the corners as
    // device positions; the gather's node CSR over the distinct chamber nodes in the caller's order, a node's corners ordered by chamber,
    // then triangle, then corner; a context with no chamber uploads nothing
    ctx->pres_blocks = ctx->pres_tris = ctx->pres_nodes = 0;
    ctx->d_pres_blk = ctx->d_pres_chm = ctx->d_pres_law = ctx->d_pres_rec = nullptr; ctx->d_pres_collapsed = ctx->d_pres_off = nullptr;
    ctx->d_pres_tri = ctx->d_pres_trichm = ctx->d_pres_node = ctx->d_pres_ptr = ctx->d_pres_stride = nullptr; ctx->d_pres_nrm = ctx->d_pres_part = nullptr;
    if (!ctx->chambers.empty()) {
        using namespace admm_dev;
        const size_t nc = ctx->chambers.size();
        size_t nt_all = 0;
        for (const admm_hip_ctx::PressureChamberHost &H : ctx->chambers) nt_all += H.tris.size() / 3;
        if (nt_all > (size_t)0x7fffffff / 3) return fail(ctx, ADMM_ERR_ARG, "pressure chambers: %zu triangles in all are more than the tables index", nt_all);
        std::vector<PresChamber> chm(nc); std::vector<PresBlock> blk; std::vector<int> tri, trichm; std::vector<NodeCsrEntry> entries;
        tri.reserve(3 * nt_all); trichm.reserve(nt_all); entries.reserve(3 * nt_all);
        for (size_t c = 0; c < nc; ++c) {
            admm_hip_ctx::PressureChamberHost &H = ctx->chambers[c];
            const int nt = (int)(H.tris.size() / 3), first = (int)trichm.size(), nb = (nt + PRES_BLOCK - 1) / PRES_BLOCK;
            chm[c] = PresChamber{first, nt, (int)blk.size(), nb, F.iperm[H.tris[0]], 0};
            for (int b = 0; b < nb; ++b) blk.push_back(PresBlock{(int)c, first + b * PRES_BLOCK});
            for (int t = 0; t < nt; ++t) {
                for (int j = 0; j < 3; ++j) { tri.push_back(F.iperm[H.tris[3 * (size_t)t + j]]); entries.push_back(NodeCsrEntry{H.tris[3 * (size_t)t + j], (long long)(first + t), (int)nt_all}); }
                trichm.push_back((int)c);
            }
            H.law_dirty = true;
        }
        const NodeCsrHost full = build_node_csr(n, entries);
        std::vector<int> node, ptr(1, 0);      // the distinct chamber nodes, compacted: device position and the run of corners
        for (int i = 0; i < n; ++i) if (full.ptr[i + 1] > full.ptr[i]) { node.push_back(F.iperm[i]); ptr.push_back(full.ptr[i + 1]); }
        ctx->pres_blocks = (int)blk.size(); ctx->pres_tris = (int)nt_all; ctx->pres_nodes = (int)node.size();
        PresBlock *db = nullptr; PresChamber *dc = nullptr; PresLaw *dl = nullptr; admm_pressure::Record *dr = nullptr;
        TRY(upload(ctx, &db, blk)); TRY(upload(ctx, &dc, chm)); TRY(dalloc(ctx, &dl, nc)); TRY(dalloc(ctx, &dr, nc)); TRY(dalloc(ctx, &ctx->d_pres_collapsed, nc));
        TRY(upload(ctx, &ctx->d_pres_tri, tri)); TRY(upload(ctx, &ctx->d_pres_trichm, trichm)); TRY(upload(ctx, &ctx->d_pres_node, node)); TRY(upload(ctx, &ctx->d_pres_ptr, ptr));
        TRY(upload(ctx, &ctx->d_pres_off, full.off)); TRY(upload(ctx, &ctx->d_pres_stride, full.stride));
        TRY(dalloc(ctx, &ctx->d_pres_nrm, 3 * nt_all)); TRY(dalloc(ctx, &ctx->d_pres_part, (size_t)admm_pressure::N_SUMS * blk.size()));
        HIPCHK(hipMemset(dl, 0, sizeof(PresLaw) * nc)); HIPCHK(hipMemset(dr, 0, sizeof(admm_pressure::Record) * nc)); HIPCHK(hipMemset(ctx->d_pres_collapsed, 0, sizeof(long long) * nc));
        HIPCHK(hipMemset(ctx->d_pres_nrm, 0, sizeof(double) * 3 * nt_all));
        ctx->d_pres_blk = db; ctx->d_pres_chm = dc; ctx->d_pres_law = dl; ctx->d_pres_rec = dr;
    }
    HIPCHK(hipDeviceSynchronize());
    ctx->info.t_upload_s = now_s() - t0;
    return ADMM_OK;
}

// contact attribution (admm_hip_enable_contact_attribution): the record of every collision element of this rank, allocated once -- by the
// switch in a finalized context, else by finalize --, and its fill: owner -1, normal 0.0
int attribution_allocate(admm_hip_ctx *ctx) {
    if (ctx->d_at_owner) return ADMM_OK;
    HIPCHK(hipSetDevice(ctx->device_id));
    long long total = 0;
    for (Batch &b : ctx->batches) if (b.kind == ADMM_KIND_COLLISION) { b.at_off = total; total += std::max(b.n_local, 1); }
    ctx->at_total = std::max(total, 1ll);
    TRY(dalloc(ctx, &ctx->d_at_normal, 3 * (size_t)ctx->at_total));
    TRY(dalloc(ctx, &ctx->d_at_owner, (size_t)ctx->at_total));
    return ADMM_OK;
}
int attribution_fill(admm_hip_ctx *ctx) {
    HIPCHK(hipSetDevice(ctx->device_id));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ctx->d_at_owner, -1, (size_t)ctx->at_total, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_at_normal, 0, sizeof(double) * 3 * (size_t)ctx->at_total, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ADMM_OK;
}

BatchDev batch_dev(const admm_hip_ctx *ctx, const Batch &b) {
    BatchDev d{};
    d.n = b.n_local; d.e0 = 0; d.e1 = b.n_local; d.keep_z = ctx->keep_z ? 1 : 0; d.idx = b.d_idx; d.rest = b.d_rest; d.par = b.d_par; d.w2h2 = b.d_w2h2; d.kblend = b.d_kblend; d.w2 = b.d_w2;
    d.u = b.d_u; d.z = b.d_z; d.state = b.d_state; d.n_iters = b.d_niters;
    d.fslot = ctx->d_fslot; d.dst = b.d_dst; d.targets = b.d_targets; d.active = b.d_active;
    d.dx_override = b.d_dx_override;
    d.order = b.d_order; d.cost = b.d_cost;
    d.res_slots = ctx->d_res_slots; d.res_partial = b.d_res_partial;
    d.pos4 = b.d_pos4; d.bn_ptr = b.d_bn_ptr; d.bn_dst = b.d_bn_dst; d.bn_end = b.d_bn_end;
    d.tpb = b.tpb;
    return d;
}

// Parity entries (admm_hip_local_step_dx, admm_hip_batch_energy_dx, admm_hip_batch_gradient_dx): the caller's D_i x rows, element-major
// [n_local][rows], in place of the batch's gather for the launches made while this object lives.  stage() transposes them to SoA,
// creates the batch's d_dx_buf at first use, queues the copy on the context's stream and sets the override; the staging vector is
// the object's until the stream has been waited for (wait(), or the destructor where no one has), and the destructor clears the
// override on every path: production launches never see it.
struct SuppliedRows {
    admm_hip_ctx *ctx; Batch &b; std::vector<double> soa; bool pending = false;
    SuppliedRows(admm_hip_ctx *c, Batch &b_) : ctx(c), b(b_) {}
    ~SuppliedRows() { if (pending) (void)hipStreamSynchronize(ctx->stream); b.d_dx_override = nullptr; }
    int stage(const double *dx) {
        const int rows = ADMM_KIND_ROWS[b.kind], n = b.n_local;
        soa.resize((size_t)rows * n);
        for (int e = 0; e < n; ++e) for (int r = 0; r < rows; ++r) soa[(size_t)r * n + e] = dx[(size_t)e * rows + r];
        if (!b.d_dx_buf) TRY(dalloc(ctx, &b.d_dx_buf, soa.size()));
        pending = true;
        HIPCHK(hipMemcpyAsync(b.d_dx_buf, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        b.d_dx_override = b.d_dx_buf;
        return ADMM_OK;
    }
    hipError_t wait() { pending = false; return hipStreamSynchronize(ctx->stream); }
};

// host SoA [rows][n] -> the caller's element-major [n][rows] (out == null: nothing)
void to_element_major(const std::vector<double> &soa, int rows, int n, double *out) {
    if (out) for (int e = 0; e < n; ++e) for (int r = 0; r < rows; ++r) out[(size_t)e * rows + r] = soa[(size_t)r * n + e];
}

FactorDev factor_dev(const admm_hip_ctx *ctx) {
    FactorDev f{};
    f.panels = ctx->d_panels; f.sn_first = ctx->d_sn_first; f.sn_ncols = ctx->d_sn_ncols; f.sn_nrows = ctx->d_sn_nrows;
    f.sn_panel_off = ctx->d_sn_panel_off; f.sn_rows_off = ctx->d_sn_rows_off; f.sn_slot_off = ctx->d_sn_slot_off;
    f.rows = ctx->d_rows; f.sn_front_off = ctx->d_sn_front_off; f.cg_ptr = ctx->d_cg_ptr; f.cg_slot = ctx->d_cg_slot; f.cg4 = (const int4 *)ctx->d_cg4;
    return f;
}
