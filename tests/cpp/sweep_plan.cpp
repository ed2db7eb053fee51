// sweep_plan.hpp executed on the CPU.  For every case: a grid Laplacian through build_symcsc, analyze and plan_panels, the plan of both
// sweeps (plan_fused_subtrees, plan_levels, plan_shard_exchange), and then the plan is RUN here the way the kernels run it -- the fused
// forward records as solve_fwd_subtree_kernel walks them, the levels' wave and block items tile by tile, the roots through
// panel_solve_host's own steps, the levels' backward items chunk by chunk, the fused backward records as bwd_record.hpp defines them
// -- and its x must EQUAL panel_solve_host's, bit for bit.
// Exact data make that possible: the panels and the right-hand side hold values from {-1, 0, 1}, both sweeps are pure multiply-add, so
// as long as every sum of a dot product's absolute terms stays below 2^40 every partial sum in every order is an integer that a double
// holds exactly.  The program checks that bound itself (every dot product it executes has the terms of one of the reference's).
// Density: a panel's diagonal entries are +-1, every other entry is non-zero with probability 1 / PANEL_SPARSITY; the largest absolute
// sum over all cases is printed at the end.
// Beside equality, what execution alone does not show: every W entry and contribution slot written exactly once, every x entry written
// exactly once, nothing read before it is written, every record inside the LDS cap and a multiple of 4 ints, every item at its level,
// every level's kernel shape one that launch_solve instantiates.
// Stand-alone: g++ tests/cpp/sweep_plan.cpp csrc/factor.cpp csrc/dense.cpp -fopenmp -I csrc; prints "sweep_plan: ok" and exits 0, or
// names each failed check.
#include "sweep_plan.hpp"

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace admm_lib;
using namespace admm_host;
using admm_dev::SweepItem;

static int failures = 0;
static const char *current = "";
#define CHECK(cond) do { if (!(cond)) { if (failures < 40) std::printf("  FAILED %s, line %d: %s\n", current, __LINE__, #cond); ++failures; } } while (0)

constexpr int PANEL_SPARSITY = 4;      // one off-diagonal panel entry in four is non-zero: the largest absolute sum over the cases below is 2^30.3 (one in three: 2^34.4, one in two: 2^38.1)
static double g_bound = 0.0;           // the largest sum of absolute terms of any dot product executed
static int g_padding = 0;              // padding items skipped (the current case)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 24); }
static double sign() { return (rnd() & 1) ? 1.0 : -1.0; }

// a sum of products with its absolute sum, three right-hand sides
struct Acc {
    double v[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
    void add(double p, const double *x) { for (int c = 0; c < 3; ++c) { v[c] += p * x[c]; a[c] += std::fabs(p * x[c]); } }
    void add(const Acc &o) { for (int c = 0; c < 3; ++c) { v[c] += o.v[c]; a[c] += o.a[c]; } }
    void done() { for (int c = 0; c < 3; ++c) g_bound = std::max(g_bound, a[c]); }
};

// ---- the meshes ----------------------------------------------------------------------------------------------------------------------
struct Mesh { int n = 0; std::vector<int> ti, tj; std::vector<double> tv, xyz; };
// an nx x ny x nz grid with the 7-point stencil (diagonals: the 27-point one), its corner at (x0, 0, 0); disconnected from what the mesh holds already
static void add_grid(Mesh &M, int nx, int ny, int nz, double x0, bool diagonals = false) {
    const int base = M.n;
    auto id = [&](int i, int j, int k) { return base + i + nx * (j + ny * k); };
    for (int k = 0; k < nz; ++k) for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) {
        const int a = id(i, j, k);
        M.xyz.push_back(x0 + i); M.xyz.push_back(j); M.xyz.push_back(k);
        M.ti.push_back(a); M.tj.push_back(a); M.tv.push_back(6.5);
        for (int dk = -1; dk <= 1; ++dk) for (int dj = -1; dj <= 1; ++dj) for (int di = -1; di <= 1; ++di) {
            const int i2 = i + di, j2 = j + dj, k2 = k + dk;
            if (i2 < 0 || i2 >= nx || j2 < 0 || j2 >= ny || k2 < 0 || k2 >= nz || id(i2, j2, k2) <= a) continue;
            if (!diagonals && std::abs(di) + std::abs(dj) + std::abs(dk) != 1) continue;
            M.ti.push_back(id(i2, j2, k2)); M.tj.push_back(a); M.tv.push_back(-1.0);
        }
    }
    M.n += nx * ny * nz;
}
static Mesh grid(int nx, int ny, int nz, bool diagonals = false) { Mesh M; add_grid(M, nx, ny, nz, 0.0, diagonals); return M; }

struct Tree { int leaf = 8, merge_above = 0; bool merge_root = false; int merge_small = 0, merge_depth = 2; };
// the factor's structure, panels from {-1, 0, 1}; b likewise (original node order), xref = panel_solve_host's x in FACTOR order
static void make_factor(const Mesh &M, const Tree &T, Factor &F, std::vector<double> &b, std::vector<double> &xref, int root_inv_min_cols = ROOT_INV_MIN_COLS) {
    SymCSC A;
    build_symcsc(M.n, M.ti, M.tj, M.tv, A);
    analyze(A, M.xyz.data(), T.leaf, F, T.merge_above, T.merge_root, T.merge_small, T.merge_depth);
    F.root_inv_min_cols = root_inv_min_cols;      // (-1: every root gets an explicit inverse, and so a place in the roots list)
    plan_panels(F);
    F.panels.assign((size_t)F.panels_size, 0.0);
    for (const Supernode &S : F.sn) {
        const int k = S.ncols, f = k + S.nrows;
        for (int j = 0; j < k; ++j) for (int i = j; i < f; ++i) F.panels[S.panel_off + i + (size_t)f * j] = (i == j || rnd() % PANEL_SPARSITY == 0) ? sign() : 0.0;
    }
    b.assign(3 * (size_t)F.n, 0.0);
    for (double &v : b) v = (double)((int)(rnd() % 3) - 1);
    std::vector<double> x(b.size());
    panel_solve_host(F, b.data(), x.data());
    xref.assign(b.size(), 0.0);
    for (int i = 0; i < F.n; ++i) for (int c = 0; c < 3; ++c) xref[3 * (size_t)i + c] = x[3 * (size_t)F.perm[i] + c];
}

// ---- what one rank holds while it sweeps ------------------------------------------------------------------------------------------
struct State {
    const Factor *F; const double *panels; const std::vector<int64_t> *poff;
    std::vector<double> y, W, C, X;      // factor order; NaN until written
    std::vector<int> wW, wC, wX;         // writes so far
    State(const Factor &F_, const double *panels_, const std::vector<int64_t> &poff_, const std::vector<double> &b) : F(&F_), panels(panels_), poff(&poff_) {
        const size_t n = (size_t)F_.n, ns = (size_t)std::max<int64_t>(F_.n_slots, 1);
        y.resize(3 * n); W.assign(3 * n, NAN); X.assign(3 * n, NAN); C.assign(3 * ns, NAN);
        wW.assign(n, 0); wX.assign(n, 0); wC.assign(ns, 0);
        for (size_t i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) y[3 * i + c] = b[3 * (size_t)F_.perm[i] + c];
    }
    void put(std::vector<double> &V, std::vector<int> &w, int64_t i, const Acc &a) { for (int c = 0; c < 3; ++c) V[3 * (size_t)i + c] = a.v[c]; ++w[(size_t)i]; }
};

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// rows [64 tile, 64 tile + 64) of a supernode's panel times its staged vector t = y_s - (contributions on its columns), as both
// wave-per-tile kernels and the block kernel compute them: in(fr) the children's contributions landing on front row fr, out(q, a) what
// becomes of contribution row q
template <class In, class Out>
static void forward_tile(State &S, int k, int r, int first, int tile, int64_t poff, In in, Out out) {
    const int f = k + r;
    std::vector<double> t(3 * (size_t)k);
    for (int j = 0; j < k; ++j) {
        Acc a; const double one = 1.0;
        a.add(one, &S.y[3 * (size_t)(first + j)]);
        Acc s = in(j);
        for (int c = 0; c < 3; ++c) { a.v[c] -= s.v[c]; a.a[c] += s.a[c]; }
        a.done();
        for (int c = 0; c < 3; ++c) t[3 * (size_t)j + c] = a.v[c];
    }
    const double *P = S.panels + poff;
    for (int i = 64 * tile; i < std::min(f, 64 * tile + 64); ++i) {
        Acc a;
        const int jend = i < k ? i + 1 : k;
        for (int j = 0; j < jend; ++j) a.add(P[i + (size_t)f * j], &t[3 * (size_t)j]);
        if (i < k) { a.done(); S.put(S.W, S.wW, first + i, a); }
        else { a.add(in(i)); a.done(); out(i - k, a); }
    }
}

// a fused forward record, walked as solve_fwd_subtree_kernel walks it; -> the contribution slots it keeps in LDS
static int forward_record(State &S, const int *rec, int64_t n_ints, int lds_cap) {
    using namespace admm_dev;
    const int nl = rec[SUB_LEVELS], item0 = rec[SUB_ITEM0], cbuf = rec[SUB_CBUF], ts = rec[SUB_TS];
    CHECK(n_ints % 4 == 0 && nl >= 1);
    CHECK(2 * (int64_t)cbuf >= n_ints && ts >= cbuf && (ts - cbuf) % 3 == 0);      // the contribution area lies behind the record, whole rows
    CHECK(8 * (ts + 3 * 64 * SUB_WAVES) <= lds_cap);
    const int nc = ts - cbuf;
    std::vector<double> cb((size_t)nc, NAN);
    std::vector<int> wlv((size_t)nc / 3, -1);      // the level that wrote a slot
    const int64_t root_slot = sub_join64(rec[SUB_ROOT_SLOT], rec[SUB_ROOT_SLOT + 1]);
    CHECK(rec[SUB_HDR] == 0 && item0 >= SUB_HDR + nl + 1);
    for (int lv = 0; lv < nl; ++lv) {
        CHECK(rec[SUB_HDR + lv] < rec[SUB_HDR + lv + 1]);
        for (int itm = rec[SUB_HDR + lv]; itm < rec[SUB_HDR + lv + 1]; ++itm) {
            const int *I = rec + item0 + SUB_ITEM * itm;
            const int k = I[SUB_K], r = I[SUB_R], first = I[SUB_FIRST], tile = I[SUB_TILE], moff = I[SUB_MAP], cdst = I[SUB_CDST];
            const int64_t poff = sub_join64(I[SUB_POFF], I[SUB_POFF + 1]);
            const int f = k + r;
            CHECK(item0 + SUB_ITEM * (itm + 1) <= n_ints && k >= 1 && k <= FWD_SMALL_KMAX && r >= 0 && 64 * tile < f);
            CHECK(moff < 0 || (moff % 4 == 0 && moff >= item0 && moff + 4 * f <= n_ints));
            auto in = [&](int fr) {
                Acc a; const double one = 1.0;
                if (moff >= 0) for (int e = 0; e < 4; ++e) {
                    const int o = rec[moff + 4 * fr + e];
                    if (o < 0) continue;
                    const bool ok = o % 3 == 0 && o + 3 <= nc && wlv[(size_t)o / 3] >= 0 && wlv[(size_t)o / 3] < lv;      // written, and by a level below
                    CHECK(ok);
                    if (ok) a.add(one, &cb[(size_t)o]);
                }
                return a;
            };
            auto out = [&](int q, const Acc &a) {
                if (cdst < 0) { S.put(S.C, S.wC, root_slot + q, a); return; }
                const int o = cdst + 3 * q;
                const bool ok = o % 3 == 0 && o + 3 <= nc && wlv[(size_t)o / 3] < 0;
                CHECK(ok);
                if (ok) { for (int c = 0; c < 3; ++c) cb[(size_t)o + c] = a.v[c]; wlv[(size_t)o / 3] = lv; }
            };
            forward_tile(S, k, r, first, tile, poff, in, out);
        }
    }
    for (int w : wlv) CHECK(w >= 0);
    return nc / 3;
}

// the children's contributions on a front row, from C (F.cg_ptr / cg_slot: the lists cg4 repeats)
static Acc front_in(State &S, int64_t fr) {
    Acc a; const double one = 1.0;
    for (int64_t g = S.F->cg_ptr[fr]; g < S.F->cg_ptr[fr + 1]; ++g) {
        const int slot = S.F->cg_slot[g];
        CHECK(S.wC[(size_t)slot] == 1);
        a.add(one, &S.C[3 * (size_t)slot]);
    }
    return a;
}
static bool padding(const SweepItem &it) { if (it.k || it.r) return false; ++g_padding; return true; }      // (the kernels' row_ok)
static void forward_item(State &S, const SweepItem &it) {
    if (padding(it)) return;
    forward_tile(S, it.k, it.r, it.first, it.part, it.panel_off, [&](int fr) { return front_in(S, it.front_off + fr); },
                 [&](int q, const Acc &a) { S.put(S.C, S.wC, it.slot_off + q, a); });
}
// a root of the roots list: panel_solve_host's forward and backward steps for it (it has no rows: x needs its own w alone)
static void sweep_root(State &S, const SweepRoot &R, const std::map<int, int> &sn_of_first) {
    const int s = sn_of_first.at(R.first);
    const Supernode &N = S.F->sn[s];
    CHECK(R.k == N.ncols && N.nrows == 0 && R.foff == N.front_off);
    const int k = N.ncols;
    forward_tile(S, k, 0, N.first, 0, (*S.poff)[s], [&](int fr) { return front_in(S, N.front_off + fr); }, [&](int, const Acc &) { CHECK(false); });
    for (int t = 1; 64 * t < k; ++t) forward_tile(S, k, 0, N.first, t, (*S.poff)[s], [&](int fr) { return front_in(S, N.front_off + fr); }, [&](int, const Acc &) { CHECK(false); });
    const double *P = S.panels + (*S.poff)[s];
    for (int j = 0; j < k; ++j) {
        Acc a;
        for (int i = j; i < k; ++i) a.add(P[i + (size_t)k * j], &S.W[3 * (size_t)(N.first + i)]);
        a.done(); S.put(S.X, S.wX, N.first + j, a);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// columns [j0, j1) of a supernode: x_j = sum_{i >= j} P_ij v_i, v = [w_s; -x(R_s)] given by row(i)
template <class Row, class Out>
static void backward_cols(State &S, int k, int f, int64_t poff, int j0, int j1, Row row, Out out) {
    const double *P = S.panels + poff;
    for (int j = j0; j < std::min(j1, k); ++j) {
        Acc a;
        for (int i = j; i < f; ++i) a.add(P[i + (size_t)f * j], row(i));
        a.done(); out(j, a);
    }
}
static void backward_item(State &S, const SweepItem &it, int cols) {
    if (padding(it)) return;
    const int *rows = S.F->rows.data() + it.rows_off;
    double neg[3];
    auto row = [&](int i) -> const double * {
        if (i < it.k) { CHECK(S.wW[(size_t)it.first + i] == 1); return &S.W[3 * (size_t)(it.first + i)]; }
        const int node = rows[i - it.k];
        CHECK(S.wX[(size_t)node] == 1);
        for (int c = 0; c < 3; ++c) neg[c] = -S.X[3 * (size_t)node + c];
        return neg;
    };
    CHECK(it.part * cols < it.k);
    backward_cols(S, it.k, it.k + it.r, it.panel_off, it.part * cols, it.part * cols + cols, row, [&](int j, const Acc &a) { S.put(S.X, S.wX, it.first + j, a); });
}
// a fused backward record: levels top-down, each staged through its stage table, then its tasks
static void backward_record(State &S, const int *rec, int64_t n_ints, int64_t panels_size, int lds_cap) {
    using namespace admm_dev;
    char msg[256];
    const bool sound = bwd_record_check(rec, n_ints, S.F->n, panels_size, msg, (int)sizeof msg);
    CHECK(sound);
    if (!sound) { std::printf("    %s\n", msg); return; }
    CHECK(n_ints % 4 == 0 && 8 * rec[BS_END] <= lds_cap);
    const int nl = rec[BS_LEVELS], mem0 = rec[BS_MEM0], task0 = rec[BS_TASK0];
    const int *lvt = rec + BS_HDR + nl + 1, *lvs = rec + BS_HDR + 2 * (nl + 1), *stage = rec + rec[BS_STAGE0];
    std::vector<double> xs((size_t)(rec[BS_VBUF] - rec[BS_XBUF]), NAN), vs((size_t)(rec[BS_END] - rec[BS_VBUF]), NAN);
    for (int lv = 0; lv < nl; ++lv) {
        for (int q = lvs[lv]; q < lvs[lv + 1]; ++q) {
            const int e = stage[q], n = -1 - e;
            double *dst = &vs[3 * (size_t)(q - lvs[lv])];
            if (e >= 0) for (int c = 0; c < 3; ++c) dst[c] = -xs[(size_t)e + c];
            else if (n & 1) { CHECK(S.wW[(size_t)(n >> 1)] == 1); for (int c = 0; c < 3; ++c) dst[c] = S.W[3 * (size_t)(n >> 1) + c]; }
            else { CHECK(S.wX[(size_t)(n >> 1)] == 1); for (int c = 0; c < 3; ++c) dst[c] = -S.X[3 * (size_t)(n >> 1) + c]; }
        }
        for (int t = lvt[lv]; t < lvt[lv + 1]; ++t) {
            const int tv = rec[task0 + t];
            const int *M = rec + mem0 + BS_MEM * (tv >> 4);
            const int k = M[BS_K], f = k + M[BS_R], j0 = 4 * (tv & 15), xoff = M[BS_XOFF];
            backward_cols(S, k, f, sub_join64(M[BS_POFF], M[BS_POFF + 1]), j0, j0 + 4, [&](int i) { return &vs[(size_t)M[BS_VOFF] + 3 * (size_t)i]; }, [&](int j, const Acc &a) {
                S.put(S.X, S.wX, M[BS_FIRST] + j, a);
                if (xoff >= 0) for (int c = 0; c < 3; ++c) xs[(size_t)xoff + 3 * (size_t)j + c] = a.v[c];
            });
        }
    }
}

// ---- one rank's plan, checked and run ------------------------------------------------------------------------------------------------
struct Reach { bool nw[17] = {}, cw[5] = {}; };      // the kernel shapes some level with items reached
struct RankPlan { FusePlan fuse; std::vector<LevelPlan> own, top; };

static RankPlan make_plan(const Factor &F, const std::vector<int64_t> &poff, int64_t psize, const std::vector<int64_t> &rinv, const std::vector<int> *own, int want,
                          const std::vector<char> &top_needed, const SweepKnobs &K, const DeviceLimits &lim) {
    RankPlan R;
    R.fuse = plan_fused_subtrees(F, poff, psize, own, want, K, lim);
    CHECK(R.fuse.error.empty());
    R.own = plan_levels(F, poff, rinv, own, want, top_needed, R.fuse.fused, R.fuse.fused_bwd, K);
    if (own) R.top = plan_levels(F, poff, rinv, own, -1, top_needed, R.fuse.fused, R.fuse.fused_bwd, K);
    return R;
}

// what execution does not show
static void check_levels(const Factor &F, const std::vector<LevelPlan> &levels, Reach &reach) {
    if (levels.empty()) return;
    CHECK(levels.size() == F.levels.size());
    for (size_t l = 0; l < levels.size(); ++l) {
        const LevelPlan &L = levels[l];
        CHECK(L.big_nw == 4 || L.big_nw == 8 || L.big_nw == 16);
        CHECK(L.bwd_cw == 4 || L.bwd_cw == 2 || L.bwd_cw == 1);
        CHECK(L.bwd_nw == 2 || L.bwd_nw == 4 || L.bwd_nw == 8 || L.bwd_nw == 16);
        CHECK(L.bwd_nw != 2 || L.bwd_cw == 4);
        CHECK(L.small.empty() || L.big.empty());
        if (!L.big.empty()) reach.nw[L.big_nw] = true;
        if (!L.bwd.empty()) reach.cw[L.bwd_cw] = true;
        for (const std::vector<SweepItem> *v : {&L.small, &L.big, &L.bwd}) for (const SweepItem &it : *v) {
            if (!it.k && !it.r) continue;
            const bool mine = it.s >= 0 && it.s < (int)F.sn.size();
            CHECK(mine);
            if (!mine) continue;
            const Supernode &N = F.sn[it.s];
            CHECK(N.level == (int)l && it.k == N.ncols && it.r == N.nrows && it.first == N.first);
            CHECK(it.front_off == N.front_off && it.slot_off == N.slot_off && it.rows_off == N.rows_off);
            if (v == &L.small) CHECK(it.k <= admm_dev::FWD_SMALL_KMAX);
        }
    }
}
static void check_records(const FusePlan &P, const DeviceLimits &lim) {
    CHECK(P.off[0] == 0 && P.off.back() == (int64_t)P.rec.size() && P.bwd_off[0] == 0 && P.bwd_off.back() == (int64_t)P.bwd_rec.size());
    CHECK(P.n_fuse_bwd() <= P.n_fuse() && P.lds <= lim.lds_cap && P.bwd_lds <= lim.lds_cap);
    int lds = 0, bwd_lds = 0;
    for (int i = 0; i < P.n_fuse(); ++i) { CHECK((P.off[i + 1] - P.off[i]) % 4 == 0 && P.off[i + 1] > P.off[i]); lds = std::max(lds, 8 * (P.rec[P.off[i] + admm_dev::SUB_TS] + 3 * 64 * admm_dev::SUB_WAVES)); }
    for (int i = 0; i < P.n_fuse_bwd(); ++i) { CHECK((P.bwd_off[i + 1] - P.bwd_off[i]) % 4 == 0 && P.bwd_off[i + 1] > P.bwd_off[i]); bwd_lds = std::max(bwd_lds, 8 * P.bwd_rec[P.bwd_off[i] + admm_dev::BS_END]); }
    CHECK(lds == P.lds && bwd_lds == P.bwd_lds);      // the launches' dynamic LDS is the largest record's
    for (size_t s = 0; s < P.fused.size(); ++s) CHECK(!P.fused_bwd[s] || P.fused[s]);
    CHECK((P.why_off != nullptr) == (P.cut < 0) && (P.why_off == nullptr || P.n_fuse() == 0) && (P.why_bwd_off != nullptr) == (P.n_fuse_bwd() == 0));
}

// the own pass of the forward sweep: the fused records, then the levels; -> contribution slots kept in LDS
static int forward_own(State &S, const RankPlan &R, const DeviceLimits &lim, const std::map<int, int> &sn_of_first) {
    int in_lds = 0;
    for (int i = 0; i < R.fuse.n_fuse(); ++i) in_lds += forward_record(S, R.fuse.rec.data() + R.fuse.off[i], R.fuse.off[i + 1] - R.fuse.off[i], lim.lds_cap);
    for (const LevelPlan &L : R.own) {
        for (const SweepItem &it : L.small) forward_item(S, it);
        for (const SweepItem &it : L.big) forward_item(S, it);
        for (const SweepRoot &r : L.roots) sweep_root(S, r, sn_of_first);
    }
    return in_lds;
}
static void forward_top(State &S, const RankPlan &R, const std::map<int, int> &sn_of_first) {
    for (const LevelPlan &L : R.top) {
        for (const SweepItem &it : L.small) forward_item(S, it);
        for (const SweepItem &it : L.big) forward_item(S, it);
        for (const SweepRoot &r : L.roots) sweep_root(S, r, sn_of_first);
    }
}
// the backward sweep in launch order: the top's levels, the own levels, the fused records
static void backward(State &S, const RankPlan &R, int64_t psize, const DeviceLimits &lim) {
    for (const std::vector<LevelPlan> *levels : {&R.top, &R.own})
        for (int l = (int)levels->size() - 1; l >= 0; --l) for (const SweepItem &it : (*levels)[l].bwd) backward_item(S, it, (*levels)[l].bwd_nw * (*levels)[l].bwd_cw);
    for (int i = 0; i < R.fuse.n_fuse_bwd(); ++i) backward_record(S, R.fuse.bwd_rec.data() + R.fuse.bwd_off[i], R.fuse.bwd_off[i + 1] - R.fuse.bwd_off[i], psize, lim.lds_cap);
}

static std::map<int, int> first_map(const Factor &F) { std::map<int, int> m; for (size_t s = 0; s < F.sn.size(); ++s) m[F.sn[s].first] = (int)s; return m; }
// does a supernode's contribution stay in the LDS of a fused forward record (a member that is not its subtree's root)?
static bool kept_in_lds(const Factor &F, const FusePlan &P, int s) { return P.fused[s] && F.sn[s].parent >= 0 && P.fused[F.sn[s].parent]; }
static bool equal_on(const std::vector<double> &a, const std::vector<double> &b, int node) { return std::memcmp(&a[3 * (size_t)node], &b[3 * (size_t)node], 3 * sizeof(double)) == 0; }

// fused forward records whose root has no contribution rows (a whole tree of a forest under the cut)
static int roots_without_rows(const FusePlan &P) {
    using namespace admm_dev;
    int n = 0;
    for (int i = 0; i < P.n_fuse(); ++i) {
        const int *rec = P.rec.data() + P.off[i];
        const int *I = rec + rec[SUB_ITEM0] + SUB_ITEM * (rec[SUB_HDR + rec[SUB_LEVELS]] - 1);      // the last item: the root's last tile
        n += I[SUB_CDST] < 0 && I[SUB_R] == 0;
    }
    return n;
}

struct Outcome { FusePlan fuse; Reach reach; int padding = 0, n_levels = 0; };

// one rank, all supernodes
static Outcome run_plain(const char *name, const Mesh &M, const Tree &T, const SweepKnobs &K, const DeviceLimits &lim, int root_inv_min_cols = ROOT_INV_MIN_COLS) {
    current = name; g_padding = 0;
    Factor F; std::vector<double> b, xref;
    make_factor(M, T, F, b, xref, root_inv_min_cols);
    const int ns = (int)F.sn.size();
    std::vector<int64_t> poff(ns), rinv(ns);
    for (int s = 0; s < ns; ++s) { poff[s] = F.sn[s].panel_off; rinv[s] = F.sn[s].root_inv_off; }
    Outcome O;
    const RankPlan R = make_plan(F, poff, F.panels_size, rinv, nullptr, 0, std::vector<char>(), K, lim);
    check_records(R.fuse, lim); check_levels(F, R.own, O.reach);
    State S(F, F.panels.data(), poff, b);
    const std::map<int, int> fm = first_map(F);
    const int in_lds = forward_own(S, R, lim, fm);
    backward(S, R, F.panels_size, lim);
    int want_lds = 0, bad_w = 0, bad_x = 0, bad_c = 0, differ = 0;
    for (int s = 0; s < ns; ++s) {
        const bool lds = kept_in_lds(F, R.fuse, s);
        if (lds) want_lds += F.sn[s].nrows;
        for (int q = 0; q < F.sn[s].nrows; ++q) bad_c += S.wC[(size_t)F.sn[s].slot_off + q] != (lds ? 0 : 1);
    }
    for (int i = 0; i < F.n; ++i) { bad_w += S.wW[i] != 1; bad_x += S.wX[i] != 1; differ += !equal_on(S.X, xref, i); }
    CHECK(in_lds == want_lds); CHECK(bad_w == 0); CHECK(bad_c == 0); CHECK(bad_x == 0); CHECK(differ == 0);
    O.fuse = R.fuse; O.padding = g_padding; O.n_levels = (int)F.levels.size();
    int roots = 0; for (const LevelPlan &L : R.own) roots += (int)L.roots.size();
    std::printf("  %-28s nodes %d supernodes %d levels %d kmax %d | cut %d fused %d left %d bwd %d (%s / %s) lds %d %d maxin %d skip %d empty %d | roots %d padding %d | %s\n", name, F.n, ns,
                (int)F.levels.size(), F.max_cols, R.fuse.cut, R.fuse.n_fuse(), R.fuse.left, R.fuse.n_fuse_bwd(), R.fuse.why_off ? R.fuse.why_off : "on", R.fuse.why_bwd_off ? R.fuse.why_bwd_off : "on",
                R.fuse.lds, R.fuse.bwd_lds, R.fuse.maxin, R.fuse.skip, R.fuse.empty, roots, g_padding, differ || bad_w || bad_c || bad_x ? "WRONG" : "equal");
    return O;
}

// Two ranks of subtree sharding with a synthetic owner: the supernodes with top[s] are the replicated top, the subtrees under it go to
// the ranks as rank_of_subtree lists them (in ascending order of their roots).  Every rank plans and sweeps with a panel layout of its
// own (its subtrees and the top, packed); the contributions of the subtrees' roots and the final x are exchanged through
// plan_shard_exchange's lists.  need_all: every rank sweeps backward over the whole top; else only over what its subtrees' rows touch.
static void run_sharded(const char *name, const Mesh &M, const Tree &T, const SweepKnobs &K, const DeviceLimits &lim, int top_depth, const std::vector<int> &rank_of_subtree, bool expect_zero) {
    current = name; g_padding = 0;
    const int world = 2;
    Factor F; std::vector<double> b, xref;
    make_factor(M, T, F, b, xref);
    const int ns = (int)F.sn.size();
    // owners: the root and what lies less than top_depth below it are the top
    std::vector<int> depth(ns, 0), sn_owner(ns, -1), node_owner(F.n, -1), sn_of(F.n, -1);
    for (int s = ns - 1; s >= 0; --s) if (F.sn[s].parent >= 0) depth[s] = depth[F.sn[s].parent] + 1;
    std::vector<int> sub_roots;
    for (int s = 0; s < ns; ++s) if (depth[s] == top_depth) sub_roots.push_back(s);
    CHECK(sub_roots.size() == rank_of_subtree.size());
    for (int s = ns - 1; s >= 0; --s) {
        if (depth[s] < top_depth) continue;
        if (depth[s] == top_depth) { const size_t q = std::find(sub_roots.begin(), sub_roots.end(), s) - sub_roots.begin(); sn_owner[s] = rank_of_subtree[std::min(q, rank_of_subtree.size() - 1)]; }
        else sn_owner[s] = sn_owner[F.sn[s].parent];
    }
    for (int s = 0; s < ns; ++s) for (int j = 0; j < F.sn[s].ncols; ++j) { node_owner[F.sn[s].first + j] = sn_owner[s]; sn_of[F.sn[s].first + j] = s; }
    // the rule of top_needs without elements: the top supernodes among the rows of a rank's subtrees, and their ancestors
    std::vector<std::vector<char> > need(world, std::vector<char>(ns, 0));
    for (int s = 0; s < ns; ++s) if (sn_owner[s] >= 0) for (int q = 0; q < F.sn[s].nrows; ++q) { const int t = sn_of[F.rows[F.sn[s].rows_off + q]]; if (sn_owner[t] < 0) need[sn_owner[s]][t] = 1; }
    for (int r = 0; r < world; ++r) for (int s = 0; s < ns; ++s) if (need[r][s] && F.sn[s].parent >= 0) need[r][F.sn[s].parent] = 1;
    std::vector<int> provider(ns, 0);
    int zeros = 0;
    for (int s = 0; s < ns; ++s) if (sn_owner[s] < 0) { provider[s] = need[0][s] ? 0 : 1; CHECK(need[0][s] || need[1][s]); zeros += !need[0][s] + !need[1][s]; }
    CHECK((zeros > 0) == expect_zero);
    const std::map<int, int> fm = first_map(F);
    std::vector<State> states; std::vector<RankPlan> plans; std::vector<ShardExchange> ex;
    std::vector<std::vector<int64_t> > poffs(world), rinvs(world); std::vector<std::vector<double> > panels(world); std::vector<int64_t> psize(world);
    Reach reach;
    for (int r = 0; r < world; ++r) {      // the compact layout of plan_device_panels
        poffs[r].assign(ns, -1); rinvs[r].assign(ns, -1);
        int64_t size = 0;
        for (int s = 0; s < ns; ++s) if (sn_owner[s] == r || sn_owner[s] < 0) {
            const int64_t len = (int64_t)(F.sn[s].ncols + F.sn[s].nrows) * F.sn[s].ncols;
            poffs[r][s] = size; panels[r].insert(panels[r].end(), F.panels.begin() + F.sn[s].panel_off, F.panels.begin() + F.sn[s].panel_off + len); size += len;
        }
        for (int s = 0; s < ns; ++s) if ((sn_owner[s] == r || sn_owner[s] < 0) && F.sn[s].root_inv_off >= 0) { rinvs[r][s] = (size + 15) & ~(int64_t)15; size = rinvs[r][s] + (int64_t)root_inv_ld(F.sn[s].ncols) * F.sn[s].ncols; }
        psize[r] = size;
    }
    states.reserve(world);
    int in_lds = 0, want_lds = 0;
    for (int r = 0; r < world; ++r) {
        plans.push_back(make_plan(F, poffs[r], psize[r], rinvs[r], &sn_owner, r, need[r], K, lim));
        check_records(plans[r].fuse, lim); check_levels(F, plans[r].own, reach); check_levels(F, plans[r].top, reach);
        for (int s = 0; s < ns; ++s) if (sn_owner[s] != r) CHECK(!plans[r].fuse.fused[s]);
        for (const LevelPlan &L : plans[r].own) for (const std::vector<SweepItem> *v : {&L.small, &L.big, &L.bwd}) for (const SweepItem &it : *v) CHECK((!it.k && !it.r) || sn_owner[it.s] == r);
        for (const LevelPlan &L : plans[r].top) for (const std::vector<SweepItem> *v : {&L.small, &L.big, &L.bwd}) for (const SweepItem &it : *v) CHECK((!it.k && !it.r) || sn_owner[it.s] < 0);
        ex.push_back(plan_shard_exchange(F, sn_owner, node_owner, provider, r));
        states.emplace_back(F, panels[r].data(), poffs[r], b);
        in_lds += forward_own(states[r], plans[r], lim, fm);
    }
    // the exchange: every rank gets the contribution rows of the other rank's subtree roots (the all-reduce of masked values)
    CHECK(ex[0].slots == ex[1].slots && ex[0].top_nodes == ex[1].top_nodes && ex[0].mine.size() == ex[0].slots.size());
    for (size_t q = 0; q < ex[0].slots.size(); ++q) {
        CHECK(ex[0].mine[q] + ex[1].mine[q] == 1);
        const int from = ex[0].mine[q] ? 0 : 1, to = 1 - from, slot = ex[0].slots[q];
        CHECK(states[from].wC[(size_t)slot] == 1 && states[to].wC[(size_t)slot] == 0);
        for (int c = 0; c < 3; ++c) states[to].C[3 * (size_t)slot + c] = states[from].C[3 * (size_t)slot + c];
        states[to].wC[(size_t)slot] = 1;
    }
    for (int i : ex[0].top_nodes) CHECK(node_owner[i] < 0);
    int bad_w = 0, bad_x = 0, bad_c = 0, differ = 0, kept = 0;
    std::vector<double> x(3 * (size_t)F.n, NAN);
    for (int r = 0; r < world; ++r) {
        State &S = states[r];
        forward_top(S, plans[r], fm);
        backward(S, plans[r], psize[r], lim);
        for (int s = 0; s < ns; ++s) {
            const bool lds = kept_in_lds(F, plans[r].fuse, s), feeds_top = sn_owner[s] >= 0 && F.sn[s].parent >= 0 && sn_owner[F.sn[s].parent] < 0;
            if (lds) want_lds += F.sn[s].nrows;
            const int want_c = sn_owner[s] == r ? (lds ? 0 : 1) : (sn_owner[s] < 0 || feeds_top ? 1 : 0);
            for (int q = 0; q < F.sn[s].nrows; ++q) bad_c += S.wC[(size_t)F.sn[s].slot_off + q] != want_c;
        }
        for (int i = 0; i < F.n; ++i) {      // W on the own subtrees and the top; x on the own subtrees and the needed top, and nowhere else
            const int o = node_owner[i];
            bad_w += S.wW[i] != ((o == r || o < 0) ? 1 : 0);
            const bool has_x = o == r || (o < 0 && need[r][sn_of[i]]);
            bad_x += S.wX[i] != (has_x ? 1 : 0);
            if (has_x) differ += !equal_on(S.X, xref, i);
            CHECK(ex[r].base[i] == ((o == r || (o < 0 && r == 0)) ? 1 : 0));
            if (ex[r].keep[i]) { CHECK(has_x); ++kept; for (int c = 0; c < 3; ++c) x[3 * (size_t)i + c] = S.X[3 * (size_t)i + c]; }
        }
    }
    for (int i = 0; i < F.n; ++i) { CHECK(ex[0].keep[i] + ex[1].keep[i] == 1); differ += !equal_on(x, xref, i); }      // the per-frame assembly of the full vector
    CHECK(kept == F.n); CHECK(in_lds == want_lds); CHECK(bad_w == 0); CHECK(bad_c == 0); CHECK(bad_x == 0); CHECK(differ == 0);
    CHECK(plans[0].fuse.n_fuse() > 0 && plans[1].fuse.n_fuse() > 0);
    std::printf("  %-28s nodes %d supernodes %d levels %d | top %d needed %d + %d | fused %d + %d bwd %d + %d | padding %d | %s\n", name, F.n, ns, (int)F.levels.size(), (int)ex[0].top_nodes.size(),
                (int)std::count(need[0].begin(), need[0].end(), 1), (int)std::count(need[1].begin(), need[1].end(), 1), plans[0].fuse.n_fuse(), plans[1].fuse.n_fuse(), plans[0].fuse.n_fuse_bwd(),
                plans[1].fuse.n_fuse_bwd(), g_padding, differ || bad_w || bad_c || bad_x ? "WRONG" : "equal");
}

int main() {
    const DeviceLimits two_cus{2, 1 << 20};      // a cut exists on small trees; LDS no limit unless a case sets one
    const SweepKnobs defaults;
    const Tree binary;
    const Mesh slab = grid(24, 24, 4), cube = grid(12, 12, 12);

    std::printf("sweep_plan: the plans, executed\n");
    // the default binary tree, and four- and eight-way ones
    Outcome o = run_plain("binary", slab, binary, defaults, two_cus);
    CHECK(o.fuse.n_fuse() >= 4 && o.fuse.n_fuse_bwd() == o.fuse.n_fuse() && o.fuse.left == 0 && o.fuse.lv_max >= 2);
    Tree four = binary; four.merge_small = 200;
    o = run_plain("four-way", slab, four, defaults, two_cus);
    CHECK(o.fuse.n_fuse() >= 4 && o.fuse.maxin >= 3);
    // (the 27-point stencil: the node where the three separators of an eight-way node meet touches all eight children)
    Tree eight = binary; eight.merge_small = 400; eight.merge_depth = 3;
    o = run_plain("eight-way, no cg4", grid(12, 12, 12, true), eight, defaults, two_cus);
    CHECK(o.fuse.why_off && std::string(o.fuse.why_off) == "front rows with more than four contributions" && o.fuse.n_fuse() == 0);
    // LDS caps: some subtrees left per-level; the backward records alone over the cap
    Outcome wide = run_plain("binary, cus 1", slab, binary, defaults, DeviceLimits{1, 1 << 20});
    CHECK(wide.fuse.n_fuse() >= 2);
    o = run_plain("small lds cap", slab, binary, defaults, DeviceLimits{1, wide.fuse.lds - 8});
    CHECK(o.fuse.left > 0 && o.fuse.n_fuse() > 0);
    {
        // A strip and a sheet of 1100 nodes each, leaves of up to 64 nodes: the two subtrees under the cut.  A backward record stages a
        // whole level at once, and the leaves' level is nearly all of the strip, so the strip's backward record needs more LDS than
        // either forward record, the sheet's less.  A cap between: both forward records fit, of the backward ones only the sheet's.
        Mesh strips = grid(550, 2, 1); add_grid(strips, 50, 22, 1, 5000.0);
        Tree fat = binary; fat.leaf = 64;
        wide = run_plain("strip and sheet", strips, fat, defaults, DeviceLimits{1, 1 << 20});
        CHECK(wide.fuse.n_fuse() == 2 && wide.fuse.n_fuse_bwd() == 2 && wide.fuse.bwd_lds > wide.fuse.lds);
        o = run_plain("... cap between fwd and bwd", strips, fat, defaults, DeviceLimits{1, (wide.fuse.lds + wide.fuse.bwd_lds) / 2});
        CHECK(o.fuse.n_fuse() == 2 && o.fuse.n_fuse_bwd() == 1 && o.fuse.left == 0);
        int both = 0, fwd_only = 0;
        for (size_t s = 0; s < o.fuse.fused.size(); ++s) { both += o.fuse.fused[s] && o.fuse.fused_bwd[s]; fwd_only += o.fuse.fused[s] && !o.fuse.fused_bwd[s]; }
        CHECK(both > 0 && fwd_only > 0);
    }
    SweepKnobs k = defaults; k.sweep_fuse = false;
    o = run_plain("sweep_fuse off", slab, binary, k, two_cus);
    CHECK(o.fuse.n_fuse() == 0 && o.fuse.why_off && o.fuse.why_bwd_off && std::string(o.fuse.why_bwd_off) == "ADMM_HIP_SWEEP_FUSE=0");
    k = defaults; k.sweep_fuse_bwd = false;
    o = run_plain("sweep_fuse_bwd off", slab, binary, k, two_cus);
    CHECK(o.fuse.n_fuse() >= 4 && o.fuse.n_fuse_bwd() == 0 && std::string(o.fuse.why_bwd_off) == "ADMM_HIP_SWEEP_FUSE_BWD=0");
    // block items low in the tree: every wave choice of the forward kernel and every column choice of the backward one
    Reach reach;
    k = defaults; k.fwd_small_k = k.bwd_small_k = 16; k.fwd_nw16_max_tiles = 2; k.fwd_nw4_kmax = 30; k.fwd_nw8_kmax = 40;
    o = run_plain("small_k 16", cube, binary, k, two_cus);
    for (int q = 0; q < 17; ++q) reach.nw[q] |= o.reach.nw[q];
    for (int q = 0; q < 5; ++q) reach.cw[q] |= o.reach.cw[q];
    k.bwd_cw2_min_cols = 40; k.bwd_cw2_max_cols = 200; k.bwd_nw_min_cols = 100; k.sweep_fuse_bwd = false;      // (... and backward items on the narrow levels)
    o = run_plain("small_k 16, cw2 lowered", cube, binary, k, two_cus);
    for (int q = 0; q < 17; ++q) reach.nw[q] |= o.reach.nw[q];
    for (int q = 0; q < 5; ++q) reach.cw[q] |= o.reach.cw[q];
    current = "kernel shapes reached";
    CHECK(reach.nw[4] && reach.nw[8] && reach.nw[16] && reach.cw[1] && reach.cw[2] && reach.cw[4]);
    // padding items
    k = defaults; k.xcd_min_supernodes = 2;
    o = run_plain("xcd order from 2 supernodes", slab, binary, k, two_cus);
    CHECK(o.padding > 0);
    k.sweep_fuse = false;
    o = run_plain("xcd order, nothing fused", slab, binary, k, two_cus);
    CHECK(o.padding > 0);
    // roots by their explicit inverse and by two sweeps
    o = run_plain("every root by its inverse", slab, binary, defaults, two_cus, -1);
    k = defaults; k.root_inverse = false;
    o = run_plain("roots by sweeps", slab, binary, k, two_cus, -1);
    // forests: whole trees under the cut, members without rows
    // (equal grids: the dissection parts them, the separator is one node of one of them, the other grid's top has no rows)
    Mesh forest = grid(12, 12, 2); add_grid(forest, 12, 12, 2, 100.0);
    o = run_plain("forest of two", forest, binary, defaults, DeviceLimits{1, 1 << 20});
    CHECK(o.fuse.n_fuse() == 2 && roots_without_rows(o.fuse) == 1);
    Mesh forest4 = forest; add_grid(forest4, 12, 12, 2, 200.0); add_grid(forest4, 12, 12, 2, 300.0);
    o = run_plain("forest of four", forest4, binary, defaults, DeviceLimits{1, 1 << 20});
    CHECK(o.fuse.n_fuse() == 2 && o.fuse.empty > 0);
    // subtree sharding
    Tree root4 = binary; root4.merge_root = true;
    run_sharded("two ranks, root is the top", slab, root4, defaults, two_cus, 1, {0, 1, 0, 1}, false);
    run_sharded("two ranks, top of three", slab, binary, defaults, two_cus, 2, {0, 0, 1, 1}, true);

    std::printf("  largest sum of absolute terms in a dot product: %.0f = 2^%.1f (every partial sum is exact below 2^53; required: below 2^40)\n", g_bound, std::log2(std::max(g_bound, 1.0)));
    current = "exactness";
    CHECK(g_bound < 1099511627776.0);      // 2^40
    if (failures) { std::printf("sweep_plan: %d checks FAILED\n", failures); return 1; }
    std::printf("sweep_plan: ok\n");
    return 0;
}
