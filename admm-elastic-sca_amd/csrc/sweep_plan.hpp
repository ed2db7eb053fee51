// sweep_plan.hpp -- the plan of both triangular sweeps as a value: which kernel shape every elimination-tree level gets, every supernode
// cut into tiles and column chunks, the LDS records of the fused subtree launches, and what a rank exchanges under subtree sharding.
// Pure functions of the factor, the knobs and two device numbers, free of HIP: upload.inc prints and uploads what they return and
// decides nothing; tests/cpp/sweep_plan.cpp includes this header alone and executes the plans on the CPU against panel_solve_host.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "factor.hpp"
#include "dev_types.hpp"
#include "fwd_record.hpp"
#include "bwd_record.hpp"

namespace admm_lib {

// what the plan reads of a context (abi_setup.inc sets it from the environment)
struct SweepKnobs {
    int fwd_small_k = 64, bwd_small_k = 64;       // levels whose widest supernode has at most this many columns: wave-per-tile forward kernel / 4 columns per wave backward
    int bwd_nw = 8, bwd_small_nw = 4;             // backward sweep, levels of wide supernodes: waves (= columns) per block sharing one staging (ADMM_HIP_BWD_NW = 4 / 8 / 16)
    int bwd_nw_min_cols = 4096;                   // ... on levels with at least this many columns, 4 below
    // backward sweep, wide levels with more columns than the chip holds waves (8 x 4 x 256) but at most twice as many: two columns per wave
    // instead of a second round of workgroups for the few that did not fit (1M-tet bar: levels 3, 4, 6, 7 with 8.6-13.7 k columns:
    // backward 0.212 -> 0.203 ms; including the top levels with 4.5-5.5 k columns: 0.229).  ADMM_HIP_BWD_CW2_MIN / _MAX, MIN 0 = off
    int bwd_cw2_min_cols = 8192, bwd_cw2_max_cols = 16384;
    int fwd_nw16_max_tiles = 512;
    int fwd_nw4_kmax = 200, fwd_nw8_kmax = 400;   // forward sweep: levels whose widest supernode has at most this many columns run 4 / 8 waves per tile (ADMM_HIP_FWD_NW4 / _NW8)
    int xcd_min_supernodes = 16;                  // levels with at least this many supernodes get the XCD-aware item order (0 = off; ADMM_HIP_XCD)
    bool root_inverse = true;                     // roots of the elimination tree: forward + backward as one product with (L L^T)^-1 (ADMM_HIP_ROOT_INVERSE=0: two sweeps)
    // the bottom subtrees of the elimination tree (every supernode up to the cut level) swept by ONE launch per sweep, one workgroup per
    // subtree, the hand-off between its levels in LDS (plan_fused_subtrees; ADMM_HIP_SWEEP_FUSE=0: per-level launches only)
    bool sweep_fuse = true;
    // ... and the backward sweep's launch over those of them whose backward record fits the LDS cap as well (bwd_record.hpp;
    // ADMM_HIP_SWEEP_FUSE_BWD=0: the backward sweep keeps its per-level launches, the forward one stays fused)
    bool sweep_fuse_bwd = true;
};

// the two numbers of the device the fused plan depends on: its compute units, and the LDS bytes a workgroup may take so that two fit a CU
struct DeviceLimits { int cus; int lds_cap; };

constexpr int BWD_BIG_CW = 1;         // backward kernel: columns per wave on levels with supernodes wider than bwd_small_k

// XCD-aware order of a level's work items.  Workgroups are dealt round-robin to the 8 XCDs (workgroup i -> XCD i mod 8), each
// with its own L2: in plain order the tiles of ONE supernode land on all eight, and every L2 fetches that supernode's staged
// vector (y, contribution lists, the children's contributions / x of its rows) from HBM again.  Here every supernode of a level
// is given to one XCD (longest first onto the least loaded) and the list is interleaved so that its items get workgroup ids of
// that XCD; queues of unequal length are padded with empty items (k = r = 0: the kernels do nothing for them).  `group` = items
// per workgroup (the wave-per-tile forward kernel packs several).  Levels with few supernodes keep the plain order: there every
// XCD is needed for each of them.
inline void xcd_order(std::vector<admm_dev::SweepItem> &items, int group, int min_supernodes) {
    const int NX = 8;
    std::vector<std::pair<int, int> > runs;      // (first item, count) per supernode; a supernode's items are consecutive
    for (size_t i = 0; i < items.size();) { size_t j = i; while (j < items.size() && items[j].s == items[i].s) ++j; runs.push_back({(int)i, (int)(j - i)}); i = j; }
    if ((int)runs.size() < min_supernodes) return;
    std::vector<int> ord(runs.size());
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return runs[a].second > runs[b].second; });
    std::vector<std::vector<admm_dev::SweepItem> > q(NX);
    for (int r : ord) {
        int best = 0;
        for (int x = 1; x < NX; ++x) if (q[x].size() < q[best].size()) best = x;
        q[best].insert(q[best].end(), items.begin() + runs[r].first, items.begin() + runs[r].first + runs[r].second);
    }
    size_t len = 0;
    for (int x = 0; x < NX; ++x) len = std::max(len, (q[x].size() + group - 1) / group * group);
    admm_dev::SweepItem none{};
    std::vector<admm_dev::SweepItem> out;
    out.reserve(len * NX);
    for (size_t g0 = 0; g0 < len; g0 += group) for (int x = 0; x < NX; ++x) for (int t = 0; t < group; ++t) out.push_back(g0 + t < q[x].size() ? q[x][g0 + t] : none);
    items.swap(out);
}

// ---- the bottom subtrees of the forward sweep, one workgroup each (solve_fwd_subtree_kernel) ---------------------------------------
// Cut level c: the highest level such that every supernode at or below it has at most 64 columns (the wave-per-tile forward and the
// 4-column backward shape) and the subtrees below it -- supernodes up to level c whose parent lies above c -- still number at least two
// per CU.  Each such subtree becomes one record, loaded into LDS once by its workgroup (fwd_record.hpp for the layout): the items of
// every level, bottom-up; per supernode with children its front map (for every front row the LDS offsets of the children's
// contribution rows landing on it, in the child order of Factor::cg4); the LDS offsets of the members' contributions.  Only the
// subtree's root writes its contribution to C.  A subtree whose LDS does not leave two workgroups per CU, the subtree of a whole tree
// (a root of the elimination tree at or below the cut) and trees whose front rows receive more than four contributions (no cg4) stay on
// the per-level path.
// ... and of the backward sweep (solve_bwd_kernel_subtree; the record's layout: bwd_record.hpp).  The backward record of the subtree under
// t, whose members bylv lists per level: the members top-down, per member its shape, where its staged vector [w_s; -x(R_s)] lies while
// its level runs, where its x is kept for the members below it (none for a member without children), and for every front row beyond
// its columns where x of that row is: in the x area (a column of a member higher up in this subtree) or in global X (above the subtree)
// -- as one stage table per level, a row of it per row of the level's staged vectors, so that the workgroup's threads share them evenly.
// One task per (member, four columns).  node_x: scratch, -1 for every node on entry and on return.  -> the workgroup's LDS bytes.
inline int bwd_subtree_record(const admm_host::Factor &F, const std::vector<int64_t> &panel_off, const std::vector<std::vector<int> > &bylv,
                              const std::vector<std::vector<int> > &children, std::vector<int> &node_x, std::vector<int> &v) {
    using namespace admm_dev;
    using admm_host::Supernode;
    std::vector<int> lvm{0}, lvt{0}, lvs{0}, mem, tasks, stage;
    int xd = 0, vmax = 0, nm = 0;
    for (int l = (int)bylv.size() - 1; l >= 0; --l) {
        if (bylv[l].empty()) continue;
        int vd = 0;
        for (int s : bylv[l]) {
            const Supernode &S = F.sn[s];
            int it[BS_MEM] = {};
            it[BS_K] = S.ncols; it[BS_R] = S.nrows; it[BS_FIRST] = S.first; it[BS_XOFF] = -1; it[BS_VOFF] = vd; it[BS_ROW0] = (int)stage.size();
            sub_split64(panel_off[s], it + BS_POFF);
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

// The fused launches of both sweeps.  rec / off: the forward records back to back and their offsets [n + 1], the largest subtree
// first; bwd_rec / bwd_off: the backward records in that same order.  fused[s] = 1 for the supernodes the fused forward launch sweeps,
// fused_bwd[s] = 1 for those of the backward launch: the members of those of the subtrees whose backward record fits the LDS cap too (a
// subset of fused: a subtree over the cap here keeps its per-level backward items only).  Every backward record passes bwd_record_check;
// error: what the check said of one that did not (nothing of the plan is to be used then).
// What ADMM_HIP_VERBOSE prints of it (tests/test_sweep_subtree*.py assert the shapes they reach from it): why_off / why_bwd_off: why a
// launch has nothing to sweep (null: it has); left: subtrees that stay on the per-level path; candidates: subtrees under the cut; the
// shapes the records reach: levels per record, the most child contributions into one front row, members whose parent lies two or more
// levels up, non-root members without contribution rows.
struct FusePlan {
    int cut = -1, lds = 0, bwd_lds = 0;      // cut level (-1: none found), dynamic LDS bytes of the two launches
    std::vector<int> rec, bwd_rec; std::vector<int64_t> off{0}, bwd_off{0};
    std::vector<char> fused, fused_bwd;
    const char *why_off = nullptr, *why_bwd_off = nullptr;
    int left = 0, candidates = 0, lv_min = 0, lv_max = 0, maxin = 0, skip = 0, empty = 0;
    std::string error;
    int n_fuse() const { return (int)off.size() - 1; }
    int n_fuse_bwd() const { return (int)bwd_off.size() - 1; }
};

// own / want: the supernodes to plan for are those with (*own)[s] == want (own null: all of them); panel_off, panels_size: where the
// device keeps every supernode's panel, and the extent of its panels (doubles)
inline FusePlan plan_fused_subtrees(const admm_host::Factor &F, const std::vector<int64_t> &panel_off, int64_t panels_size, const std::vector<int> *own, int want,
                                    const SweepKnobs &knobs, const DeviceLimits &limits) {
    using namespace admm_dev;
    using admm_host::Supernode;
    const int ns = (int)F.sn.size();
    FusePlan P;
    P.fused.assign(ns, 0); P.fused_bwd.assign(ns, 0);
    const char *why_bwd_off = !knobs.sweep_fuse ? "ADMM_HIP_SWEEP_FUSE=0" : (!knobs.sweep_fuse_bwd ? "ADMM_HIP_SWEEP_FUSE_BWD=0" : (F.n > BS_MAX_NODES ? "too many nodes" : nullptr));
    auto off = [&](const char *why) { P.why_off = why; P.why_bwd_off = why_bwd_off ? why_bwd_off : "no fused forward subtrees"; return P; };
    if (!knobs.sweep_fuse) return off("ADMM_HIP_SWEEP_FUSE=0");
    if (F.cg4.empty()) return off("front rows with more than four contributions");
    auto mine = [&](int s) { return !own || (*own)[s] == want; };
    const int lds_cap = limits.lds_cap;
    const int kcap = std::min(std::min(knobs.fwd_small_k, knobs.bwd_small_k), FWD_SMALL_KMAX);
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
        if (roots >= 2 * limits.cus) cut = l;
    }
    if (cut < 0) return off("no cut level");
    P.cut = cut;
    std::vector<std::vector<int> > children(ns);
    for (int s = 0; s < ns; ++s) if (F.sn[s].parent >= 0) children[F.sn[s].parent].push_back(s);
    std::vector<int> local_slot(F.n_slots, -1);      // member's contribution slot -> LDS offset (doubles, from the contribution area)
    struct Rec { std::vector<int> v; double bytes; std::vector<int> members; std::vector<int> bwd; };      // (bwd: empty = per-level backward items)
    std::vector<Rec> recs;
    std::vector<int> node_x(F.n, -1);      // (bwd_subtree_record's scratch)
    int n_bwd = 0;
    for (int t = 0; t < ns; ++t) {
        const int p = F.sn[t].parent;
        if (!mine(t) || F.sn[t].level > cut || p < 0 || F.sn[p].level <= cut) continue;
        ++P.candidates;
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
                sub_split64(panel_off[s], it + SUB_POFF);
                for (int tile = 0; tile < (f + 63) / 64; ++tile) {
                    it[SUB_TILE] = tile;
                    items.insert(items.end(), it, it + SUB_ITEM);
                    ++n_items;
                }
            }
            lvp.push_back(n_items);
        }
        for (int s : mem) if (s != t) for (int q = 0; q < F.sn[s].nrows; ++q) local_slot[F.sn[s].slot_off + q] = -1;
        if (!ok) { ++P.left; continue; }
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
        if (lds > lds_cap) { ++P.left; continue; }
        double bytes = 0.0;
        for (int s : mem) { const double k = F.sn[s].ncols, f = k + F.sn[s].nrows; bytes += 8.0 * (f * k - 0.5 * k * (k - 1)); }
        P.lds = std::max(P.lds, lds);
        P.lv_min = recs.empty() ? nl : std::min(P.lv_min, nl); P.lv_max = std::max(P.lv_max, nl);
        for (size_t q = 0; q < maps.size(); q += 4) P.maxin = std::max(P.maxin, (maps[q] >= 0) + (maps[q + 1] >= 0) + (maps[q + 2] >= 0) + (maps[q + 3] >= 0));
        for (int s : mem) if (s != t) { P.skip += F.sn[F.sn[s].parent].level - F.sn[s].level >= 2; P.empty += F.sn[s].nrows == 0; }
        std::vector<int> bwd;
        if (!why_bwd_off) {
            const int bl = bwd_subtree_record(F, panel_off, bylv, children, node_x, bwd);
            if (bl > lds_cap) bwd.clear();
            else {
                char msg[256];
                if (!bwd_record_check(bwd.data(), (int64_t)bwd.size(), F.n, panels_size, msg, (int)sizeof msg)) { P.error = msg; return P; }
                P.bwd_lds = std::max(P.bwd_lds, bl); ++n_bwd;
            }
        }
        recs.push_back({std::move(v), bytes, std::move(mem), std::move(bwd)});
    }
    P.why_bwd_off = why_bwd_off ? why_bwd_off : (n_bwd ? nullptr : (recs.empty() ? "no fused forward subtrees" : "every subtree over the LDS cap"));
    // the largest subtrees start first, in both launches
    std::stable_sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.bytes > b.bytes; });
    for (const Rec &r : recs) {
        P.rec.insert(P.rec.end(), r.v.begin(), r.v.end()); P.off.push_back((int64_t)P.rec.size());
        for (int s : r.members) P.fused[s] = 1;
        if (r.bwd.empty()) continue;
        P.bwd_rec.insert(P.bwd_rec.end(), r.bwd.begin(), r.bwd.end()); P.bwd_off.push_back((int64_t)P.bwd_rec.size());
        for (int s : r.members) P.fused_bwd[s] = 1;
    }
    return P;
}

// ---- the per-level launches ---------------------------------------------------------------------------------------------------------
// One level of one pass.  Per level, by its widest supernode: forward as wave items (one wave per 64-row tile, k <= fwd_small_k <= 64)
// or block items (big_nw waves split a tile's columns); backward with 4 columns per wave (k <= bwd_small_k), otherwise BWD_BIG_CW (2 on
// levels whose column count lies in (bwd_cw2_min_cols, bwd_cw2_max_cols]), bwd_nw waves per block: an item of `bwd` is bwd_nw * bwd_cw
// columns of a supernode.  roots: solved with their explicit inverse -- gather + one row-wise product, no items in either list.
struct SweepRoot { int k, first; int64_t foff, inv_off; };
struct LevelPlan {
    std::vector<admm_dev::SweepItem> small, big, bwd;
    std::vector<SweepRoot> roots;
    int big_nw = 16, bwd_cw = 1, bwd_nw = 4;
    double mbytes = 0.0;      // (diagnostics: panel bytes of this level's supernodes)
};

// One pass over the levels: the supernodes with (*own)[s] == want (own null: all of them; want < 0: the replicated top of subtree
// sharding, which has no fused subtrees and sweeps backward only over the separators with top_needed[s]).  fused / fused_bwd
// (plan_fused_subtrees): no per-level items in the forward / the backward sweep.
inline std::vector<LevelPlan> plan_levels(const admm_host::Factor &F, const std::vector<int64_t> &panel_off, const std::vector<int64_t> &root_inv_off, const std::vector<int> *own,
                                          int want, const std::vector<char> &top_needed, const std::vector<char> &fused, const std::vector<char> &fused_bwd, const SweepKnobs &knobs) {
    using admm_dev::SweepItem;
    using admm_host::Supernode;
    const int fwd_small_k = std::min(knobs.fwd_small_k, admm_dev::FWD_SMALL_KMAX);
    std::vector<LevelPlan> levels(F.levels.size());
    for (size_t l = 0; l < F.levels.size(); ++l) {
        LevelPlan &L = levels[l];
        int level_kmax = 0;
        for (int s : F.levels[l]) level_kmax = std::max(level_kmax, F.sn[s].ncols);
        const bool fwd_small = level_kmax <= fwd_small_k, bwd_small = level_kmax <= knobs.bwd_small_k;
        L.bwd_cw = bwd_small ? 4 : BWD_BIG_CW;   // columns per wave in the backward kernel
        // eight columns per block pay where a level has thousands of columns (one staging of the vector per 8 instead of 4
        // columns); on levels with few columns the larger number of blocks matters more (50k-tet bar: 4 waves 222 us / 8: 228)
        int level_cols = 0;
        for (int s : F.levels[l]) if (!own || (*own)[s] == want) level_cols += F.sn[s].ncols;
        L.bwd_nw = bwd_small ? knobs.bwd_small_nw : (level_cols >= knobs.bwd_nw_min_cols ? knobs.bwd_nw : 4);
        if (!bwd_small && knobs.bwd_cw2_min_cols > 0 && level_cols > knobs.bwd_cw2_min_cols && level_cols <= knobs.bwd_cw2_max_cols) L.bwd_cw = 2;
        for (int s : F.levels[l]) {
            if (own && (*own)[s] != want) continue;
            const Supernode &S = F.sn[s];
            SweepItem it{};
            it.s = s; it.k = S.ncols; it.r = S.nrows; it.first = S.first;
            it.panel_off = panel_off[s]; it.front_off = S.front_off; it.slot_off = S.slot_off; it.rows_off = S.rows_off;
            const int f = S.ncols + S.nrows;
            const int tiles = (f + 63) / 64;
            L.mbytes += 8e-6 * ((double)f * S.ncols - 0.5 * (double)S.ncols * (S.ncols - 1));
            if (S.root_inv_off >= 0 && knobs.root_inverse) {      // a root: x = (L L^T)^-1 t in the forward sweep, nothing in the backward sweep
                L.roots.push_back({S.ncols, S.first, S.front_off, root_inv_off[s]});
                continue;
            }
            const bool in_fused = want >= 0 && fused[s];
            if (!in_fused) for (int t = 0; t < tiles; ++t) { it.part = t; if (fwd_small) L.small.push_back(it); else L.big.push_back(it); }
            const int chunks = (S.ncols + L.bwd_nw * L.bwd_cw - 1) / (L.bwd_nw * L.bwd_cw);
            if (own && want < 0 && !top_needed[s]) continue;      // replicated top: no backward work for a separator this rank never reads
            if (want >= 0 && fused_bwd[s]) continue;
            for (int c = 0; c < chunks; ++c) { it.part = c; L.bwd.push_back(it); }
        }
        if (knobs.xcd_min_supernodes > 0) { xcd_order(L.small, admm_dev::FWD_SMALL_WAVES, knobs.xcd_min_supernodes); xcd_order(L.big, 1, knobs.xcd_min_supernodes); xcd_order(L.bwd, 1, knobs.xcd_min_supernodes); }
        int kmax = 0;
        for (const SweepItem &q : L.big) kmax = std::max(kmax, q.k);
        // few tiles (all resident at once even with 16 waves each): the more waves share a tile's columns the shorter its chain
        L.big_nw = (int)L.big.size() <= knobs.fwd_nw16_max_tiles ? 16 : (kmax <= knobs.fwd_nw4_kmax ? 4 : (kmax <= knobs.fwd_nw8_kmax ? 8 : 16));
    }
    return levels;
}

// ---- subtree sharding: the exchange lists (see shard_pack_kernel) and the node masks -------------------------------------------------
// top_nodes: the nodes of the replicated top; slots / mine: the contribution rows of the owned subtrees' roots, which feed the top, and
// whether this rank computes them; base: the nodes whose right-hand side base term this rank adds; keep: the nodes whose x this rank
// gives to the per-frame assembly of the full vector (x of a top node comes from top_provider, the lowest rank that computes it)
struct ShardExchange {
    std::vector<int> top_nodes, slots;
    std::vector<unsigned char> mine, base, keep;
};
inline ShardExchange plan_shard_exchange(const admm_host::Factor &F, const std::vector<int> &sn_owner, const std::vector<int> &node_owner, const std::vector<int> &top_provider, int rank) {
    const int ns = (int)F.sn.size();
    ShardExchange E;
    E.base.resize(F.n); E.keep.resize(F.n);
    for (int i = 0; i < F.n; ++i) {
        const int o = node_owner[i];
        if (o < 0) E.top_nodes.push_back(i);
        E.base[i] = E.keep[i] = (o == rank || (o < 0 && rank == 0)) ? 1 : 0;
    }
    for (int s = 0; s < ns; ++s) if (sn_owner[s] < 0)      // x of a top node comes from the lowest rank that computes it
        for (int j = 0; j < F.sn[s].ncols; ++j) E.keep[F.sn[s].first + j] = top_provider[s] == rank ? 1 : 0;
    for (int s = 0; s < ns; ++s) {      // roots of the owned subtrees: their contribution rows feed the top
        const int par = F.sn[s].parent;
        if (sn_owner[s] < 0 || par < 0 || sn_owner[par] >= 0) continue;
        for (int q = 0; q < F.sn[s].nrows; ++q) { E.slots.push_back((int)(F.sn[s].slot_off + q)); E.mine.push_back(sn_owner[s] == rank ? 1 : 0); }
    }
    return E;
}

} // namespace admm_lib
