// upload.inc -- the factor and the batches on the device: sweep work items per level, SoA element arrays, RHS slot layout
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
// ---- the bottom subtrees of the forward sweep, one workgroup each (solve_fwd_subtree_kernel) ---------------------------------------
// Cut level c: the highest level such that every supernode at or below it has at most 64 columns (the wave-per-tile forward and the
// 4-column backward shape) and the subtrees below it -- supernodes up to level c whose parent lies above c -- still number at least two
// per CU.  Each such subtree becomes one record, loaded into LDS once by its workgroup (admm_dev::SUB_* for the layout): the items of
// every level, bottom-up; per supernode with children its front map (for every front row the LDS offsets of the children's
// contribution rows landing on it, in the child order of Factor::cg4); the LDS offsets of the members' contributions.  Only the
// subtree's root writes its contribution to C.  A subtree whose LDS does not leave two workgroups per CU, the subtree of a whole tree
// (a root of the elimination tree at or below the cut) and trees whose front rows receive more than four contributions (no cg4) stay on
// the per-level path.  fused[s] = 1 for the supernodes the fused launch sweeps.  ADMM_HIP_VERBOSE: one "plan fused" line per call, early returns
// included (tests/test_sweep_subtree*.py assert the shapes they reach from it).
// ... and of the backward sweep (solve_bwd_kernel_subtree; the record's layout: bwd_record.hpp).  The backward record of the subtree under
// t, whose members bylv lists per level: the members top-down, per member its shape, where its staged vector [w_s; -x(R_s)] lies while
// its level runs, where its x is kept for the members below it (none for a member without children), and for every front row beyond
// its columns where x of that row is: in the x area (a column of a member higher up in this subtree) or in global X (above the subtree)
// -- as one stage table per level, a row of it per row of the level's staged vectors, so that the workgroup's threads share them evenly.
// One task per (member, four columns).  node_x: scratch, -1 for every node on entry and on return.  -> the workgroup's LDS bytes.
int bwd_subtree_record(const admm_hip_ctx *ctx, const std::vector<std::vector<int> > &bylv, const std::vector<std::vector<int> > &children, std::vector<int> &node_x,
                       std::vector<int> &v) {
    using namespace admm_dev;
    const Factor &F = ctx->F;
    std::vector<int> lvm{0}, lvt{0}, lvs{0}, mem, tasks, stage;
    int xd = 0, vmax = 0, nm = 0;
    for (int l = (int)bylv.size() - 1; l >= 0; --l) {
        if (bylv[l].empty()) continue;
        int vd = 0;
        for (int s : bylv[l]) {
            const Supernode &S = F.sn[s];
            int it[BS_MEM] = {};
            it[BS_K] = S.ncols; it[BS_R] = S.nrows; it[BS_FIRST] = S.first; it[BS_XOFF] = -1; it[BS_VOFF] = vd; it[BS_ROW0] = (int)stage.size();
            sub_split64(ctx->dev_panel_off[s], it + BS_POFF);
            vd += 3 * (S.ncols + S.nrows);
            for (int j = 0; j < S.ncols; ++j) stage.push_back(-1 - (2 * (S.first + j) + 1));
            for (int q = 0; q < S.nrows; ++q) { const int node = F.rows[S.rows_off + q]; stage.push_back(node_x[node] >= 0 ? node_x[node] : -1 - 2 * node); }
            if (!children[s].empty()) {
                it[BS_XOFF] = xd;
                for (int j = 0; j < S.ncols; ++j) node_x[S.first + j] = xd + 3 * j;
                xd += 3 * S.ncols;
            }
            for (int g = 0; 4 * g < S.ncols; ++g) tasks.push_back(nm * 16 + g);
            mem.insert(mem.end(), it, it + BS_MEM);
            ++nm;
        }
        vmax = std::max(vmax, vd);
        lvm.push_back(nm); lvt.push_back((int)tasks.size()); lvs.push_back((int)stage.size());
    }
    for (const std::vector<int> &lv : bylv) for (int s : lv) if (!children[s].empty()) for (int j = 0; j < F.sn[s].ncols; ++j) node_x[F.sn[s].first + j] = -1;
    const int nl = (int)lvm.size() - 1;
    const int mem0 = (BS_HDR + 3 * (nl + 1) + 3) & ~3, task0 = mem0 + BS_MEM * nm, stage0 = task0 + (int)tasks.size();
    const int n_ints = (stage0 + (int)stage.size() + 3) & ~3;
    v.assign(n_ints, 0);
    const int xbuf = n_ints / 2, vbuf = xbuf + xd, end = vbuf + vmax;      // (doubles)
    v[BS_LEVELS] = nl; v[BS_NMEM] = nm; v[BS_MEM0] = mem0; v[BS_NTASK] = (int)tasks.size(); v[BS_TASK0] = task0; v[BS_XBUF] = xbuf; v[BS_VBUF] = vbuf; v[BS_END] = end;
    v[BS_NSTAGE] = (int)stage.size(); v[BS_STAGE0] = stage0;
    for (int l = 0; l <= nl; ++l) { v[BS_HDR + l] = lvm[l]; v[BS_HDR + nl + 1 + l] = lvt[l]; v[BS_HDR + 2 * (nl + 1) + l] = lvs[l]; }
    std::copy(mem.begin(), mem.end(), v.begin() + mem0);
    std::copy(tasks.begin(), tasks.end(), v.begin() + task0);
    std::copy(stage.begin(), stage.end(), v.begin() + stage0);
    return 8 * end;
}

// fused_bwd[s] = 1 for the supernodes the fused backward launch sweeps: the members of those of the subtrees above whose backward record fits the
// LDS cap too (a subset of fused: a subtree over the cap here keeps its per-level backward items only).  Every backward record passes
// bwd_record_check before it is uploaded.  ADMM_HIP_VERBOSE: one "plan fused_bwd" line per call beside the "plan fused" one.
int fuse_subtrees(admm_hip_ctx *ctx, const std::vector<int> *own, int want, std::vector<char> &fused, std::vector<char> &fused_bwd) {
    using namespace admm_dev;
    const Factor &F = ctx->F;
    const int ns = (int)F.sn.size();
    fused.assign(ns, 0); fused_bwd.assign(ns, 0);
    ctx->fuse_cut = -1; ctx->n_fuse = 0; ctx->fuse_lds = 0;
    ctx->n_fuse_bwd = 0; ctx->fuse_bwd_lds = 0;
    const bool verbose = getenv("ADMM_HIP_VERBOSE") != nullptr;
    const char *why_bwd_off = !ctx->sweep_fuse ? "ADMM_HIP_SWEEP_FUSE=0" : (!ctx->sweep_fuse_bwd ? "ADMM_HIP_SWEEP_FUSE_BWD=0" : (F.n > BS_MAX_NODES ? "too many nodes" : nullptr));
    auto bwd_off = [&](const char *why) { if (verbose) fprintf(stderr, "admm_hip: plan fused_bwd off (%s)\n", why); };
    const char *why_off = !ctx->sweep_fuse ? "ADMM_HIP_SWEEP_FUSE=0" : (F.cg4.empty() ? "front rows with more than four contributions" : (F.levels.empty() ? "no cut level" : nullptr));
    if (why_off) { if (verbose) fprintf(stderr, "admm_hip: plan fused off (%s)\n", why_off); bwd_off(why_bwd_off ? why_bwd_off : "no fused forward subtrees"); return ADMM_OK; }
    auto mine = [&](int s) { return !own || (*own)[s] == want; };
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ctx->device_id));
    const int cus = std::max(prop.multiProcessorCount, 1);
    const int lds_cap = (int)std::min<size_t>(prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor / 2);
    const int kcap = std::min(std::min(ctx->fwd_small_k, ctx->bwd_small_k), FWD_SMALL_KMAX);
    int cut = -1;
    for (int l = 0; l < (int)F.levels.size(); ++l) {
        bool narrow = true;
        for (int s : F.levels[l]) if (mine(s) && F.sn[s].ncols > kcap) narrow = false;
        if (!narrow) break;
        int roots = 0;
        for (int s = 0; s < ns; ++s) {
            const int p = F.sn[s].parent;
            if (mine(s) && F.sn[s].level <= l && p >= 0 && F.sn[p].level > l) ++roots;
        }
        if (roots >= 2 * cus) cut = l;
    }
    if (cut < 0) { if (verbose) fprintf(stderr, "admm_hip: plan fused off (no cut level)\n"); bwd_off(why_bwd_off ? why_bwd_off : "no fused forward subtrees"); return ADMM_OK; }
    std::vector<std::vector<int> > children(ns);
    for (int s = 0; s < ns; ++s) if (F.sn[s].parent >= 0) children[F.sn[s].parent].push_back(s);
    std::vector<int> local_slot(F.n_slots, -1);      // member's contribution slot -> LDS offset (doubles, from the contribution area)
    struct Rec { std::vector<int> v; double bytes; std::vector<int> members; std::vector<int> bwd; };      // (bwd: empty = per-level backward items)
    std::vector<Rec> recs;
    int lds_max = 0, left = 0;      // (left: subtrees that stay on the per-level path)
    std::vector<int> node_x(F.n, -1);      // (bwd_subtree_record's scratch)
    int bwd_lds_max = 0, n_bwd = 0, candidates = 0;
    // the shapes the fused records reach (ADMM_HIP_VERBOSE only): levels per record, the most child contributions into one front row,
    // members whose parent lies two or more levels up, non-root members without contribution rows
    int lv_min = 0, lv_max = 0, maxin = 0, skip = 0, empty = 0;
    for (int t = 0; t < ns; ++t) {
        const int p = F.sn[t].parent;
        if (!mine(t) || F.sn[t].level > cut || p < 0 || F.sn[p].level <= cut) continue;
        ++candidates;
        std::vector<int> mem, stack{t};      // the subtree, then per level
        while (!stack.empty()) { const int s = stack.back(); stack.pop_back(); mem.push_back(s); for (int c : children[s]) stack.push_back(c); }
        const int nlv = F.sn[t].level + 1;
        std::vector<std::vector<int> > bylv(nlv);
        for (int s : mem) bylv[F.sn[s].level].push_back(s);
        for (auto &v : bylv) std::sort(v.begin(), v.end());
        bool ok = true;
        for (int s : mem) if (!mine(s) || F.sn[s].root_inv_off >= 0) ok = false;
        // layout: header, level pointers, items, front maps; then (in LDS) the members' contributions and the waves' staged vectors
        int cdoubles = 0;
        for (int s : mem) if (s != t) { for (int q = 0; q < F.sn[s].nrows; ++q) local_slot[F.sn[s].slot_off + q] = cdoubles + 3 * q; cdoubles += 3 * F.sn[s].nrows; }
        std::vector<int> lvp{0}, items, maps;
        int n_items = 0;
        for (int l = 0; l < nlv; ++l) {
            if (bylv[l].empty()) continue;
            for (int s : bylv[l]) {
                const Supernode &S = F.sn[s];
                const int f = S.ncols + S.nrows;
                int moff = -1;
                if (!children[s].empty()) {
                    moff = (int)maps.size();
                    for (int fr = 0; fr < f; ++fr) for (int e = 0; e < 4; ++e) {
                        const int g = F.cg4[4 * (size_t)(S.front_off + fr) + e];
                        const int o = g < 0 ? -1 : local_slot[g];
                        if (g >= 0 && o < 0) ok = false;
                        maps.push_back(o);
                    }
                }
                const int cdst = s == t ? -1 : (S.nrows ? local_slot[S.slot_off] : 0);      // (-1: the root, to C)
                int it[SUB_ITEM] = {};
                it[SUB_K] = S.ncols; it[SUB_R] = S.nrows; it[SUB_FIRST] = S.first; it[SUB_MAP] = moff; it[SUB_CDST] = cdst;
                sub_split64(ctx->dev_panel_off[s], it + SUB_POFF);
                for (int tile = 0; tile < (f + 63) / 64; ++tile) {
                    it[SUB_TILE] = tile;
                    items.insert(items.end(), it, it + SUB_ITEM);
                    ++n_items;
                }
            }
            lvp.push_back(n_items);
        }
        for (int s : mem) if (s != t) for (int q = 0; q < F.sn[s].nrows; ++q) local_slot[F.sn[s].slot_off + q] = -1;
        if (!ok) { ++left; continue; }
        const int nl = (int)lvp.size() - 1;
        const int item0 = (SUB_HDR + nl + 1 + 3) & ~3, map0 = item0 + SUB_ITEM * n_items;
        const int n_ints = (map0 + (int)maps.size() + 3) & ~3;
        std::vector<int> v(n_ints, 0);
        const int64_t rs = F.sn[t].slot_off;
        const int cbuf = n_ints / 2;      // (doubles)
        const int ts_off = cbuf + cdoubles;
        v[SUB_LEVELS] = nl; v[SUB_ITEM0] = item0; v[SUB_CBUF] = cbuf; v[SUB_TS] = ts_off; sub_split64(rs, &v[SUB_ROOT_SLOT]);
        for (int l = 0; l <= nl; ++l) v[SUB_HDR + l] = lvp[l];
        for (size_t q = 0; q < items.size(); ++q) {
            v[item0 + q] = items[q];
            if (q % SUB_ITEM == SUB_MAP && items[q] >= 0) v[item0 + q] += map0;      // front map: offset in the record
        }
        std::copy(maps.begin(), maps.end(), v.begin() + map0);
        const int lds = 8 * (ts_off + 3 * 64 * SUB_WAVES);
        if (lds > lds_cap) { ++left; continue; }
        double bytes = 0.0;
        for (int s : mem) { const double k = F.sn[s].ncols, f = k + F.sn[s].nrows; bytes += 8.0 * (f * k - 0.5 * k * (k - 1)); }
        lds_max = std::max(lds_max, lds);
        if (verbose) {
            lv_min = recs.empty() ? nl : std::min(lv_min, nl); lv_max = std::max(lv_max, nl);
            for (size_t q = 0; q < maps.size(); q += 4) maxin = std::max(maxin, (maps[q] >= 0) + (maps[q + 1] >= 0) + (maps[q + 2] >= 0) + (maps[q + 3] >= 0));
            for (int s : mem) if (s != t) { skip += F.sn[F.sn[s].parent].level - F.sn[s].level >= 2; empty += F.sn[s].nrows == 0; }
        }
        std::vector<int> bwd;
        if (!why_bwd_off) {
            const int bl = bwd_subtree_record(ctx, bylv, children, node_x, bwd);
            if (bl > lds_cap) bwd.clear();
            else {
                char msg[256];
                if (!bwd_record_check(bwd.data(), (int64_t)bwd.size(), F.n, ctx->dev_panels_size, msg, (int)sizeof msg)) return fail(ctx, ADMM_ERR_STATE, "%s", msg);
                bwd_lds_max = std::max(bwd_lds_max, bl); ++n_bwd;
            }
        }
        recs.push_back({std::move(v), bytes, std::move(mem), std::move(bwd)});
    }
    if (verbose)
        fprintf(stderr, "admm_hip: plan fused cut %d subtrees %d left %d lds %d cap %d levels %d..%d maxin %d skip %d empty %d\n", cut, (int)recs.size(), left, lds_max, lds_cap,
                lv_min, lv_max, maxin, skip, empty);
    if (why_bwd_off) bwd_off(why_bwd_off);
    else if (!n_bwd) bwd_off(recs.empty() ? "no fused forward subtrees" : "every subtree over the LDS cap");
    else if (verbose) fprintf(stderr, "admm_hip: plan fused_bwd cut %d subtrees %d left %d lds %d cap %d\n", cut, n_bwd, candidates - n_bwd, bwd_lds_max, lds_cap);
    if (recs.empty()) return ADMM_OK;
    // the largest subtrees start first
    std::stable_sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.bytes > b.bytes; });
    std::vector<int> all; std::vector<int64_t> off{0};
    for (const Rec &r : recs) { all.insert(all.end(), r.v.begin(), r.v.end()); off.push_back((int64_t)all.size()); for (int s : r.members) fused[s] = 1; }
    TRY(upload(ctx, &ctx->d_fuse_rec, all)); TRY(upload(ctx, &ctx->d_fuse_off, off));
    ctx->fuse_cut = cut; ctx->n_fuse = (int)recs.size(); ctx->fuse_lds = lds_max;
    if (n_bwd) {      // (in the forward launch's order: the largest subtrees start first)
        std::vector<int> ball; std::vector<int64_t> boff{0};
        for (const Rec &r : recs) if (!r.bwd.empty()) { ball.insert(ball.end(), r.bwd.begin(), r.bwd.end()); boff.push_back((int64_t)ball.size()); for (int s : r.members) fused_bwd[s] = 1; }
        TRY(upload(ctx, &ctx->d_fuse_bwd_rec, ball)); TRY(upload(ctx, &ctx->d_fuse_bwd_off, boff));
        ctx->n_fuse_bwd = n_bwd; ctx->fuse_bwd_lds = bwd_lds_max;
    }
    return ADMM_OK;
}

int upload_factor(admm_hip_ctx *ctx) {
#ifdef ADMM_SWEEP_PROFILE
    g_swp_wgs = 0; g_swp_meta.clear();
#endif
    Factor &F = ctx->F;
    const int ns = (int)F.sn.size();
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
    ctx->levels.assign(F.levels.size(), LevelDev());
    // Per level, by its widest supernode: forward as wave items (one wave per 64-row tile, k <= fwd_small_k <= 64) or block
    // items (NW waves split a tile's columns); backward with 4 columns per wave (k <= bwd_small_k), otherwise BWD_BIG_CW
    // (2 on levels whose column count lies in (bwd_cw2_min_cols, bwd_cw2_max_cols]).
    std::vector<int> level_kmax(F.levels.size(), 0);
    for (size_t l = 0; l < F.levels.size(); ++l) for (int s : F.levels[l]) level_kmax[l] = std::max(level_kmax[l], F.sn[s].ncols);
    const int fwd_small_k = std::min(ctx->fwd_small_k, admm_dev::FWD_SMALL_KMAX);
    const bool subtree = ctx->shard_mode == 1 && ctx->world > 1;
    ctx->levels_top.assign(subtree ? F.levels.size() : 0, LevelDev());
    // passes: (which supernodes, into which list).  Plain: all -> levels.  Subtree sharding: this rank's -> levels, the replicated
    // top -> levels_top.
    struct Pass { int want; std::vector<LevelDev> *into; };
    std::vector<Pass> passes;
    if (subtree) { passes.push_back({ctx->rank, &ctx->levels}); passes.push_back({-1, &ctx->levels_top}); }
    else passes.push_back({0, &ctx->levels});
    const std::vector<int> *own = subtree ? &ctx->sn_owner : nullptr;
    std::vector<char> fused, fused_bwd;      // supernodes of the fused bottom subtrees (this rank's own ones under subtree sharding): no per-level items in the forward / the backward sweep
    TRY(fuse_subtrees(ctx, own, subtree ? ctx->rank : 0, fused, fused_bwd));
    // Subtree sharding: which top supernodes' x does a rank need?  The forward sweep over the top is complete on every rank (it sums
    // towards the root), but the backward sweep only has to reach the separators a rank touches: those that appear among the front rows
    // of its own subtrees, those its elements have a node in, and their ancestors.  Everybody evaluates the rule for EVERY rank (no
    // communication): a top supernode's x goes into the per-frame assembly of the full vector from the lowest rank that computes it.
    std::vector<char> top_needed;                 // this rank's
    std::vector<int> top_provider;
    if (subtree) {
        std::vector<std::vector<char> > need;
        top_needs(ctx, need, top_provider);      // (partition.cpp)
        top_needed = need[ctx->rank];
        if (getenv("ADMM_HIP_VERBOSE")) {
            int nt = 0, nn = 0;
            for (int s2 = 0; s2 < ns; ++s2) if (ctx->sn_owner[s2] < 0) { ++nt; nn += top_needed[s2] ? 1 : 0; }
            fprintf(stderr, "admm_hip: rank %d: backward sweep over %d of the %d top supernodes\n", ctx->rank, nn, nt);
        }
    }
    for (const Pass &ps : passes) {
        for (size_t l = 0; l < F.levels.size(); ++l) {
            LevelDev &L = (*ps.into)[l];
            std::vector<admm_dev::SweepItem> sm, bg, bw;
            L.level = (int)l; L.mbytes = 0.0;
            const bool fwd_small = level_kmax[l] <= fwd_small_k, bwd_small = level_kmax[l] <= ctx->bwd_small_k;
            L.bwd_cw = bwd_small ? 4 : BWD_BIG_CW;   // columns per wave in the backward kernel
            // eight columns per block pay where a level has thousands of columns (one staging of the vector per 8 instead of 4
            // columns); on levels with few columns the larger number of blocks matters more (50k-tet bar: 4 waves 222 us / 8: 228)
            int level_cols = 0;
            for (int s : F.levels[l]) if (!own || (*own)[s] == ps.want) level_cols += F.sn[s].ncols;
            L.bwd_nw = bwd_small ? ctx->bwd_small_nw : (level_cols >= ctx->bwd_nw_min_cols ? ctx->bwd_nw : 4);
            if (!bwd_small && ctx->bwd_cw2_min_cols > 0 && level_cols > ctx->bwd_cw2_min_cols && level_cols <= ctx->bwd_cw2_max_cols) L.bwd_cw = 2;
            for (int s : F.levels[l]) {
                if (own && (*own)[s] != ps.want) continue;
                const Supernode &S = F.sn[s];
                admm_dev::SweepItem it{};
                it.s = s; it.k = S.ncols; it.r = S.nrows; it.first = S.first;
                it.panel_off = ctx->dev_panel_off[s]; it.front_off = S.front_off; it.slot_off = S.slot_off; it.rows_off = S.rows_off;
                const int f = S.ncols + S.nrows;
                const int tiles = (f + 63) / 64;
                L.mbytes += 8e-6 * ((double)f * S.ncols - 0.5 * (double)S.ncols * (S.ncols - 1));
                if (S.root_inv_off >= 0 && ctx->root_inverse) {      // a root: x = (L L^T)^-1 t in the forward sweep, nothing in the backward sweep
                    L.roots.push_back({S.ncols, S.first, S.front_off, ctx->dev_root_inv_off[s]});
                    continue;
                }
                const bool in_fused = ps.want >= 0 && fused[s];
                if (!in_fused) for (int t = 0; t < tiles; ++t) { it.part = t; if (fwd_small) sm.push_back(it); else bg.push_back(it); }
                const int chunks = (S.ncols + L.bwd_nw * L.bwd_cw - 1) / (L.bwd_nw * L.bwd_cw);
                if (subtree && ps.want < 0 && !top_needed[s]) continue;      // replicated top: no backward work for a separator this rank never reads
                if (ps.want >= 0 && fused_bwd[s]) continue;
                for (int c = 0; c < chunks; ++c) { it.part = c; bw.push_back(it); }
            }
            if (ctx->xcd_min_supernodes > 0) { xcd_order(sm, admm_dev::FWD_SMALL_WAVES, ctx->xcd_min_supernodes); xcd_order(bg, 1, ctx->xcd_min_supernodes); xcd_order(bw, 1, ctx->xcd_min_supernodes); }
            L.n_small = (int)sm.size(); L.n_big = (int)bg.size(); L.n_bwd = (int)bw.size();
            int kmax = 0;
            for (const admm_dev::SweepItem &q : bg) kmax = std::max(kmax, q.k);
            // few tiles (all resident at once even with 16 waves each): the more waves share a tile's columns the shorter its chain
            L.big_nw = (int)bg.size() <= ctx->fwd_nw16_max_tiles ? 16 : (kmax <= ctx->fwd_nw4_kmax ? 4 : (kmax <= ctx->fwd_nw8_kmax ? 8 : 16));
            if (getenv("ADMM_HIP_VERBOSE")) {
                // the sweep plan of this level (tests/test_wide_supernodes.py asserts from it which kernel paths a scene reaches): column
                // chunks of the widest block item, row chunks of the tallest front in the backward kernel, and per root its product's chunks
                using namespace admm_dev;
                const char *pass = ps.want < 0 ? "top" : "own";
                const int kchunk = L.big_nw == 16 ? FwdBig<16>::KCHUNK : (L.big_nw == 8 ? FwdBig<8>::KCHUNK : FwdBig<4>::KCHUNK);
                int fmax = 0;
                for (const SweepItem &q : bw) fmax = std::max(fmax, q.k + q.r);
                fprintf(stderr, "admm_hip: plan %s level %zu: fwd wave %d block %d big_nw %d kmax %d chunks %d | bwd cw %d nw %d items %d fmax %d rchunks %d | cg4 %d\n",
                        pass, l, L.n_small, L.n_big, L.big_nw, kmax, (kmax + kchunk - 1) / kchunk, L.bwd_cw, L.bwd_nw, L.n_bwd, fmax, (fmax + BWD_RCHUNK - 1) / BWD_RCHUNK,
                        F.cg4.empty() ? 0 : 1);
                for (const LevelDev::Root &R : L.roots)
                    fprintf(stderr, "admm_hip: plan %s level %zu: root k %d %s chunks %d\n", pass, l, R.k, R.k <= ctx->root_fuse_k ? "fused" : "gather",
                            (R.k + ROOT_KCHUNK - 1) / ROOT_KCHUNK);
            }
#ifdef ADMM_SWEEP_PROFILE
            {
                const int list = ps.want < 0 ? 100 : (&ps - &passes[0]);
                auto reg = [&](std::vector<admm_dev::SweepItem> &v, int group, int tag) {
                    if (v.empty()) return;
                    const int n_wg = ((int)v.size() + group - 1) / group;
                    for (size_t i = 0; i < v.size(); ++i) v[i].pad2 = (v[i].k || v[i].r) ? (long long)(g_swp_wgs + i / group) : -1;
                    for (int q : {tag, (int)l, n_wg, (int)(L.mbytes * 1024), list, (int)g_swp_wgs}) g_swp_meta.push_back(q);
                    g_swp_wgs += n_wg;
                };
                reg(sm, admm_dev::FWD_SMALL_WAVES, 0); reg(bg, 1, L.big_nw); reg(bw, 1, 100 + 10 * L.bwd_cw + (L.bwd_nw == 16 ? 6 : L.bwd_nw));
            }
#endif
            TRY(upload(ctx, &L.d_small, sm)); TRY(upload(ctx, &L.d_big, bg)); TRY(upload(ctx, &L.d_bwd, bw));
        }
    }
    if (subtree && ctx->dist_top && getenv("ADMM_HIP_VERBOSE"))      // (the top's per-level lines above are not run: the root's rows are this rank's product)
        fprintf(stderr, "admm_hip: plan dist-top rank %d: root k %d rows %d..%d nrows %d chunks %d\n", ctx->rank, ctx->root_k, ctx->root_r0, ctx->root_r1,
                ctx->root_r1 - ctx->root_r0, (ctx->root_k + admm_dev::ROOT_KCHUNK - 1) / admm_dev::ROOT_KCHUNK);
#ifdef ADMM_SWEEP_PROFILE
    {
        unsigned long long *p = nullptr;
        TRY(dalloc(ctx, (double **)&p, 4 * g_swp_wgs + 4));
        HIPCHK(hipMemset(p, 0, sizeof(unsigned long long) * (4 * g_swp_wgs + 4)));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(admm_dev::g_sweep_prof), &p, sizeof(p)));
        g_swp_base = p;
    }
#endif
    // subtree sharding: the exchange lists (see shard_pack_kernel) and the node masks
    ctx->n_comm_top = ctx->n_comm_slots = 0;
    ctx->d_comm_top = ctx->d_comm_slots = nullptr; ctx->d_comm_mine = ctx->d_base_mask = ctx->d_keep_mask = nullptr; ctx->d_comm_buf = nullptr;
    if (subtree) {
        std::vector<int> top_nodes, slots; std::vector<unsigned char> mine, base(F.n), keep(F.n);
        for (int i = 0; i < F.n; ++i) {
            const int o = ctx->node_owner[i];
            if (o < 0) top_nodes.push_back(i);
            base[i] = keep[i] = (o == ctx->rank || (o < 0 && ctx->rank == 0)) ? 1 : 0;
        }
        for (int s2 = 0; s2 < ns; ++s2) if (ctx->sn_owner[s2] < 0)      // x of a top node comes from the lowest rank that computes it
            for (int j = 0; j < F.sn[s2].ncols; ++j) keep[F.sn[s2].first + j] = top_provider[s2] == ctx->rank ? 1 : 0;
        for (int s = 0; s < ns; ++s) {      // roots of the owned subtrees: their contribution rows feed the top
            const int par = F.sn[s].parent;
            if (ctx->sn_owner[s] < 0 || par < 0 || ctx->sn_owner[par] >= 0) continue;
            for (int q = 0; q < F.sn[s].nrows; ++q) { slots.push_back((int)(F.sn[s].slot_off + q)); mine.push_back(ctx->sn_owner[s] == ctx->rank ? 1 : 0); }
        }
        ctx->n_comm_top = (int)top_nodes.size(); ctx->n_comm_slots = (int)slots.size();
        TRY(upload(ctx, &ctx->d_comm_top, top_nodes)); TRY(upload(ctx, &ctx->d_comm_slots, slots)); TRY(upload(ctx, &ctx->d_comm_mine, mine));
        TRY(upload(ctx, &ctx->d_base_mask, base)); TRY(upload(ctx, &ctx->d_keep_mask, keep));
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
    HIPCHK(hipDeviceSynchronize());
    ctx->info.t_upload_s = now_s() - t0;
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
