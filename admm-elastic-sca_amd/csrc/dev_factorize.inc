// dev_factorize.inc -- numeric multifrontal factorization on the GPU (factor_dev.hpp kernels), System.cpp:138-140 / 167-179
// (a part of the device translation unit admm_hip.hip: the kernels can live in one translation unit only)

// ---- numeric factorization on the device (factor_dev.hpp) -------------------------------------------------------------
// The symbolic structure (ctx->F: supernodes, rows, levels) is the host's; this fills ctx->d_panels.  Every call builds the task
// records against freshly allocated fronts (all fronts of a phase resident at once: sum f^2 doubles, 4.0 GB at the 1M-tet bar), runs the
// launches level by level on the context's stream and frees the fronts again.  Returns ADMM_DEVFACTOR_NOFIT (> 0, internal)
// when the fronts do not fit: the caller then factors on the host as before.
//
// Rank-local mode (ctx->factor_local_on: subtree shards, world > 1): the reference's one solver.compute(A) (System.cpp:138-140) split
// across the ranks instead of repeated on each.  A front depends on A's columns of its supernode and on its children's update
// matrices only, so
//   phase 1  this rank's own subtrees, bottom-up, exactly as on one GPU (fronts and panels of nobody else's supernodes exist here);
//   exchange the update matrix of every subtree root whose parent lies in the replicated top goes, lower triangle packed, into its
//            place in ONE buffer that is zero elsewhere; ONE all-reduce through the installed transport (x + 0 + ... + 0: exact in any
//            order) leaves every rank with every root's update matrix -- the same bits everywhere;
//   phase 2  the top, bottom-up, on every rank alike: extend-add from top children's fronts and from the buffer in the tree's fixed
//            child order => the top's panels are bitwise identical on all ranks (and bitwise those of the whole factorization).
//            Distributed top (ctx->dist_top): the top is ONE root supernode; its front and L^-1 (k^2 doubles each) are temporaries of this
//            phase, what stays on the device is this rank's rows [root_r0, root_r1) of (L L^T)^-1 (gemm with K_FROM_MAX + koff).
// The own subtrees' fronts are freed before the top's are allocated (peak = the larger phase).  The call is collective in this mode (admm_hip_finalize / admm_hip_recompute_weights: see admm_hip_set_factor_local).
//   outcome  one more all-reduce of `world` doubles, which every rank reaches whatever its phases did: every rank returns the same code and,
//            for a matrix that is not positive definite, names the same supernode (a non-positive pivot in one rank's subtrees is not only its own).
constexpr int ADMM_DEVFACTOR_NOFIT = 1000;
// contexts of ONE process that share a device (the N-ranks-on-one-GPU tests and tools) factor their own subtrees one after the other: a rank's
// fronts are the memory peak of its initialize, and they are gone again before the next rank's arrive.  One context per process: never contended.
static std::mutex g_own_fronts_mutex;

int device_factorize(admm_hip_ctx *ctx) {
    using namespace admm_dev;
    const double t0 = now_s();
    Factor &F = ctx->F;
    const int ns = (int)F.sn.size();
    const bool local = ctx->factor_local_on;
    const int me = ctx->rank;
    hipStream_t st = ctx->stream;
    auto is_mine = [&](int s) { return !local || ctx->sn_owner[s] == me; };
    auto is_top = [&](int s) { return local && ctx->sn_owner[s] < 0; };
    // fronts of the two phases (one rank: everything is phase 1) and, rank-local, the exchanged update matrices (EVERY rank's subtree roots
    // below the top), packed lower triangles
    int64_t ftot_own = 0, ftot_top = 0, xtot = 0;
    std::vector<int64_t> xoff(ns, -1);
    for (int s = 0; s < ns; ++s) {
        const int64_t f = F.sn[s].ncols + F.sn[s].nrows;
        if (is_mine(s)) ftot_own += f * f; else if (is_top(s)) ftot_top += f * f;
        const int par = F.sn[s].parent;
        if (local && ctx->sn_owner[s] >= 0 && par >= 0 && ctx->sn_owner[par] < 0 && F.sn[s].nrows > 0) { xoff[s] = xtot; xtot += (int64_t)F.sn[s].nrows * (F.sn[s].nrows + 1) / 2; }
    }
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // the fronts of the larger phase plus this call's side buffers (A's values and scatter maps: ~20 bytes per entry; row maps; the task records)
    const double side_b = 20.0 * (double)ctx->A.val.size() + 4.0 * (double)F.rows.size() + 64.0 * 1024.0 * 1024.0;
    const int64_t root_tmp = ctx->dist_top ? (int64_t)ctx->root_k * ctx->root_k : 0;      // distributed top: the root's L^-1, a temporary next to its front
    int nofit = ((double)(std::max(ftot_own, ftot_top + root_tmp) + xtot) * 8.0 + side_b > 0.8 * (double)free_b) ? 1 : 0;
    if (nofit && !local) return ADMM_DEVFACTOR_NOFIT;
    double *d_xbuf = nullptr, *d_aval = nullptr, *d_cons = nullptr; int *d_rel = nullptr, *d_fail = nullptr;
    auto cleanup = [&]() { for (void *p : {(void *)d_xbuf, (void *)d_aval, (void *)d_cons, (void *)d_rel, (void *)d_fail}) if (p) (void)hipFree(p); };
    const int world = ctx->world;
    if (local) {
        if (!nofit && xtot && hipMalloc(&d_xbuf, sizeof(double) * xtot) != hipSuccess) { (void)hipGetLastError(); d_xbuf = nullptr; nofit = 1; }
        // "does not fit" must be every rank's decision or nobody's: the ranks meet in a collective further down.  One more tiny all-reduce
        // (through the same transport) makes it a consensus.  d_cons: [0] this flag, [1, 1 + world) every rank's outcome (the consensus at the end)
        double h_flag = (double)nofit;
        if (hipMalloc(&d_cons, sizeof(double) * (1 + world)) != hipSuccess) { cleanup(); (void)hipGetLastError(); return fail(ctx, ADMM_ERR_HIP, "device factorization: no memory for the consensus flag"); }
        int rc = hipMemcpyAsync(d_cons, &h_flag, sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess ? ADMM_OK : ADMM_ERR_HIP;
        if (!rc) rc = do_allreduce(ctx, d_cons, 1);
        if (!rc) rc = (hipMemcpyAsync(&h_flag, d_cons, sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) ? ADMM_OK : ADMM_ERR_HIP;
        if (rc) { cleanup(); return rc == ADMM_ERR_HIP ? fail(ctx, ADMM_ERR_HIP, "device factorization: consensus all-reduce failed") : rc; }
        if (h_flag > 0.0) nofit = 1;
    }
    if (nofit) { cleanup(); return ADMM_DEVFACTOR_NOFIT; }
    // an allocation that fails is "does not fit" (clean up, clear HIP's error, let the caller factor on the host); anything else is an error
    // (rank-local mode: past the consensus above an allocation failure is an error -- the other ranks are on their way to the collective)
#define DF_CHK(call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory && !local) { cleanup(); (void)hipGetLastError(); return ADMM_DEVFACTOR_NOFIT; } \
                          if (e_ != hipSuccess) { cleanup(); return fail(ctx, ADMM_ERR_HIP, "device factorization: %s: %s", #call, hipGetErrorString(e_)); } } while (0)
    // the supernode of every (factor-order) column; a child's update rows in its parent's front
    std::vector<int> sn_of(std::max(F.n, 1), 0);
    for (int s = 0; s < ns; ++s) for (int j = 0; j < F.sn[s].ncols; ++j) sn_of[F.sn[s].first + j] = s;
    std::vector<int> rel(std::max<size_t>(F.rows.size(), 1), 0);
    std::vector<std::vector<int> > kids(ns);
    for (int s = 0; s < ns; ++s) {
        const Supernode &S = F.sn[s];
        if (S.parent < 0) continue;
        kids[S.parent].push_back(s);
        if (!is_mine(S.parent) && !is_top(S.parent)) continue;
        const Supernode &Pn = F.sn[S.parent];
        const int *prow = F.rows.data() + Pn.rows_off, *rows = F.rows.data() + S.rows_off;
        for (int a = 0; a < S.nrows; ++a) {
            const int row = rows[a];
            rel[S.rows_off + a] = row < Pn.first + Pn.ncols ? row - Pn.first : Pn.ncols + (int)(std::lower_bound(prow, prow + Pn.nrows, row) - prow);
        }
    }
    if (d_xbuf) DF_CHK(hipMemsetAsync(d_xbuf, 0, sizeof(double) * xtot, st));
    DF_CHK(hipMemsetAsync(ctx->d_panels, 0, sizeof(double) * std::max<int64_t>(ctx->dev_panels_size, 1), st));
    DF_CHK(hipMalloc(&d_aval, sizeof(double) * std::max<size_t>(ctx->A.val.size(), 1)));
    DF_CHK(hipMalloc(&d_rel, sizeof(int) * rel.size()));
    DF_CHK(hipMalloc(&d_fail, sizeof(int)));
    DF_CHK(hipMemcpyAsync(d_aval, ctx->A.val.data(), sizeof(double) * ctx->A.val.size(), hipMemcpyHostToDevice, st));
    DF_CHK(hipMemcpyAsync(d_rel, rel.data(), sizeof(int) * rel.size(), hipMemcpyHostToDevice, st));
    DF_CHK(hipMemsetAsync(d_fail, 0, sizeof(int), st));
    double *Pn = ctx->d_panels;
    const std::vector<int64_t> &poff = ctx->dev_panel_off;
    double flop = 0.0, t_kernels = 0.0; size_t n_launches = 0, n_gemm = 0, n_potrf = 0, n_ext = 0;
    const bool verbose = getenv("ADMM_HIP_VERBOSE") != nullptr;

    // ---- one phase: the fronts of the supernodes `want` selects -- allocate, assemble, factor level by level, (pack_roots: the own subtree roots'
    //      update matrices into the exchange buffer), free.  Returns 0, ADMM_DEVFACTOR_NOFIT or an error code.
    auto phase = [&](const std::function<bool(int)> &want, int64_t ftot, bool pack_roots) -> int {
        const double tp = now_s();
        std::vector<int64_t> foff(ns, -1);
        { int64_t o = 0; for (int s = 0; s < ns; ++s) if (want(s)) { const int64_t f = F.sn[s].ncols + F.sn[s].nrows; foff[s] = o; o += f * f; } }
        // A's entries -> their places in the fronts, straight from A in the caller's order (one pass, no permuted copy of the matrix: an entry (i, j)
        // lands in the front of the supernode that holds the smaller of the two factor-order indices, at the row of the larger one; the scatter's
        // order does not matter).  Entries of supernodes this phase does not hold are skipped -- a rank touches its share of A only.
        std::vector<int64_t> adst; std::vector<int> asrc;
        {
            const SymCSC &A = ctx->A;
            for (int j = 0; j < A.n; ++j) {
                const int b = F.iperm[j];
                for (int64_t p = A.ptr[j]; p < A.ptr[j + 1]; ++p) {
                    const int a = F.iperm[A.idx[p]];
                    const int col = std::min(a, b), row = std::max(a, b);
                    const int sn = sn_of[col];
                    if (!want(sn)) continue;
                    const Supernode &S = F.sn[sn];
                    const int k = S.ncols, f = k + S.nrows;
                    const int *rows = F.rows.data() + S.rows_off;
                    const int loc = row < S.first + k ? row - S.first : k + (int)(std::lower_bound(rows, rows + S.nrows, row) - rows);
                    adst.push_back(foff[sn] + loc + (int64_t)f * (col - S.first)); asrc.push_back((int)p);
                }
            }
        }
        const int64_t nnz = (int64_t)adst.size();
        const double t_maps = now_s() - tp;
        double *d_fronts = nullptr, *d_rootP = nullptr; int64_t *d_adst = nullptr; int *d_asrc = nullptr;
        GemmTask *d_gemm = nullptr; PotrfTask *d_potrf = nullptr; ExtendTask *d_ext = nullptr; PackTask *d_pack = nullptr;
        auto pfree = [&]() { for (void *p : {(void *)d_fronts, (void *)d_rootP, (void *)d_adst, (void *)d_asrc, (void *)d_gemm, (void *)d_potrf, (void *)d_ext, (void *)d_pack}) if (p) (void)hipFree(p); };
#define PH_CHK(call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory && !local) { pfree(); (void)hipGetLastError(); return (int)ADMM_DEVFACTOR_NOFIT; } \
                          if (e_ != hipSuccess) { pfree(); return fail(ctx, ADMM_ERR_HIP, "device factorization: %s: %s", #call, hipGetErrorString(e_)); } } while (0)
        PH_CHK(hipMalloc(&d_fronts, sizeof(double) * std::max<int64_t>(ftot, 1)));
        PH_CHK(hipMemsetAsync(d_fronts, 0, sizeof(double) * std::max<int64_t>(ftot, 1), st));
        // distributed top: the root's L^-1 (k x k) lives only as long as this phase -- what stays is this rank's rows of (L L^T)^-1
        const int droot = (ctx->dist_top && want(ctx->root_sn)) ? ctx->root_sn : -1;
        if (droot >= 0) {
            const size_t kk = (size_t)F.sn[droot].ncols * F.sn[droot].ncols;
            PH_CHK(hipMalloc(&d_rootP, sizeof(double) * std::max<size_t>(kk, 1)));
            PH_CHK(hipMemsetAsync(d_rootP, 0, sizeof(double) * std::max<size_t>(kk, 1), st));
        }
        auto panel = [&](int s) { return s == droot ? d_rootP : Pn + poff[s]; };
        PH_CHK(hipMalloc(&d_adst, sizeof(int64_t) * std::max<int64_t>(nnz, 1)));
        PH_CHK(hipMalloc(&d_asrc, sizeof(int) * std::max<int64_t>(nnz, 1)));
        PH_CHK(hipMemcpyAsync(d_adst, adst.data(), sizeof(int64_t) * nnz, hipMemcpyHostToDevice, st));
        PH_CHK(hipMemcpyAsync(d_asrc, asrc.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, st));
        // task records and the launch sequence
        std::vector<GemmTask> gemm; std::vector<PotrfTask> potrf; std::vector<ExtendTask> ext; std::vector<PackTask> pack;
        struct Launch { int kind, first, count, gx; };      // kind 0 extend-add, 1 potrf + block inverse, 2 gemm, 3 pack
        std::vector<Launch> launches;
        auto front = [&](int s) { return d_fronts + foff[s]; };
        auto close_gemm = [&](size_t first) {
            if (gemm.size() == first) return;
            int gx = 1;
            for (size_t q = first; q < gemm.size(); ++q) gx = std::max(gx, ((gemm[q].m + 63) / 64) * ((gemm[q].n + 63) / 64));
            launches.push_back({2, (int)first, (int)(gemm.size() - first), gx});
        };
        auto add_gemm = [&](const double *A, int lda, const double *B, int ldb, double *C, int ldc, int m, int n, int k, int flags, double alpha, double beta) {
            if (m <= 0 || n <= 0 || k <= 0) return;
            GemmTask T{}; T.A = A; T.B = B; T.C = C; T.m = m; T.n = n; T.k = k; T.lda = lda; T.ldb = ldb; T.ldc = ldc; T.flags = flags; T.alpha = alpha; T.beta = beta;
            gemm.push_back(T);
        };
        for (size_t l = 0; l < F.levels.size(); ++l) {
            std::vector<int> lev;
            for (int s : F.levels[l]) if (want(s)) lev.push_back(s);
            if (lev.empty()) continue;
            // extend-add, one launch per child rank (two children of one front never in the same launch: fixed summation order)
            size_t max_kids = 0; for (int s : lev) max_kids = std::max(max_kids, kids[s].size());
            for (size_t q = 0; q < max_kids; ++q) {
                const size_t first = ext.size(); int gx = 1;
                for (int s : lev) {
                    if (kids[s].size() <= q) continue;
                    const int c = kids[s][q]; const Supernode &Cn = F.sn[c];
                    if (Cn.nrows == 0) continue;
                    const int fc = Cn.ncols + Cn.nrows;
                    ExtendTask T{}; T.P = front(s); T.rel = d_rel + Cn.rows_off; T.rc = Cn.nrows; T.fc = fc; T.fp = F.sn[s].ncols + F.sn[s].nrows;
                    if (xoff[c] >= 0) { T.U = d_xbuf + xoff[c]; T.packed = 1; }      // a subtree root below the top: from the exchanged buffer (on its owner too)
                    else T.U = front(c) + Cn.ncols + (size_t)fc * Cn.ncols;
                    ext.push_back(T); gx = std::max(gx, (Cn.nrows + 7) / 8);
                }
                if (ext.size() > first) launches.push_back({0, (int)first, (int)(ext.size() - first), gx});
            }
            int kmax = 0; for (int s : lev) kmax = std::max(kmax, F.sn[s].ncols);
            for (int jb = 0; jb < kmax; jb += 64) {
                const size_t pfirst = potrf.size();
                for (int s : lev) {
                    const Supernode &S = F.sn[s]; const int k = S.ncols, f = k + S.nrows;
                    if (k <= jb) continue;
                    PotrfTask T{}; T.w = std::min(64, k - jb); T.ld = f; T.ldo = f; T.id = s;
                    T.blk = front(s) + jb + (size_t)f * jb; T.out = panel(s) + jb + (size_t)f * jb;
                    potrf.push_back(T);
                }
                launches.push_back({1, (int)pfirst, (int)(potrf.size() - pfirst), 1});
                size_t gfirst = gemm.size();
                for (int s : lev) {      // F[below, J] <- F[below, J] Dinv^T
                    const Supernode &S = F.sn[s]; const int k = S.ncols, f = k + S.nrows;
                    if (k <= jb) continue;
                    const int w = std::min(64, k - jb);
                    double *X = front(s) + (jb + w) + (size_t)f * jb;
                    add_gemm(X, f, panel(s) + jb + (size_t)f * jb, f, X, f, f - jb - w, w, w, GEMM_TRANS_B, 1.0, 0.0);
                }
                close_gemm(gfirst);
                gfirst = gemm.size();
                for (int s : lev) {      // F[below, below] -= F[below, J] F[below, J]^T (lower tiles)
                    const Supernode &S = F.sn[s]; const int k = S.ncols, f = k + S.nrows;
                    if (k <= jb) continue;
                    const int w = std::min(64, k - jb);
                    const double *X = front(s) + (jb + w) + (size_t)f * jb;
                    add_gemm(X, f, X, f, front(s) + (jb + w) + (size_t)f * (jb + w), f, f - jb - w, f - jb - w, w, GEMM_TRANS_B | GEMM_LOWER_TILES, -1.0, 1.0);
                }
                close_gemm(gfirst);
            }
            // P[0:k, 0:k] = L11^-1 from the block inverses, by doubling: X[bottom, top] = -X[bottom, bottom] (L[bottom, top] X[top, top]);
            // the inner product lands (transposed) in the unused upper triangle of the front
            const int nbmax = (kmax + 63) / 64;
            for (int half = 1; half < nbmax; half *= 2) {
                for (int pass = 0; pass < 2; ++pass) {
                    const size_t gfirst = gemm.size();
                    for (int s : lev) {
                        const Supernode &S = F.sn[s]; const int k = S.ncols, f = k + S.nrows, nb = (k + 63) / 64;
                        for (int gb = 0; gb + half < nb; gb += 2 * half) {
                            const int g0 = 64 * gb, sz = 64 * half, h = std::min(k, 64 * (gb + 2 * half)) - (g0 + sz);
                            double *Tt = front(s) + g0 + (size_t)f * (g0 + sz);      // (sz x h): transpose of L[bottom, top] X[top, top]
                            double *Ps = panel(s);
                            if (pass == 0) add_gemm(Ps + g0 + (size_t)f * g0, f, front(s) + (g0 + sz) + (size_t)f * g0, f, Tt, f, sz, h, sz, GEMM_TRANS_A | GEMM_TRANS_B, 1.0, 0.0);
                            else add_gemm(Ps + (g0 + sz) + (size_t)f * (g0 + sz), f, Tt, f, Ps + (g0 + sz) + (size_t)f * g0, f, h, sz, h, GEMM_TRANS_B, -1.0, 0.0);
                        }
                    }
                    close_gemm(gfirst);
                }
            }
            {      // P[k:f, :] = L21 L11^-1
                const size_t gfirst = gemm.size();
                for (int s : lev) {
                    const Supernode &S = F.sn[s]; const int k = S.ncols, f = k + S.nrows;
                    add_gemm(front(s) + k, f, panel(s), f, panel(s) + k, f, S.nrows, k, k, GEMM_K_FROM_COL, 1.0, 0.0);
                }
                close_gemm(gfirst);
            }
        }
        {      // roots: (L L^T)^-1 = L^-T L^-1, full symmetric
            const size_t gfirst = gemm.size();
            for (int s = 0; s < ns; ++s) {
                const Supernode &S = F.sn[s];
                if (!want(s) || ctx->dev_root_inv_off[s] < 0) continue;
                const int k = S.ncols;
                if (s == droot) {      // this rank's rows [r0, r1) of the symmetric inverse = its columns [r0, r1): C = L^-T L^-1[:, r0:r1]
                    const int r0 = ctx->root_r0, nr = ctx->root_r1 - ctx->root_r0;
                    add_gemm(panel(s), k, panel(s) + (size_t)k * r0, k, Pn + ctx->dev_root_inv_off[s], root_inv_ld(k), k, nr, k, GEMM_TRANS_A | GEMM_K_FROM_MAX, 1.0, 0.0);
                    if (nr > 0) gemm.back().koff = r0;
                    continue;
                }
                add_gemm(Pn + poff[s], k, Pn + poff[s], k, Pn + ctx->dev_root_inv_off[s], root_inv_ld(k), k, k, k, GEMM_TRANS_A | GEMM_K_FROM_MAX, 1.0, 0.0);
            }
            close_gemm(gfirst);
        }
        if (pack_roots) {      // the own subtree roots' update matrices into the exchange buffer
            int gx = 1;
            for (int s = 0; s < ns; ++s) {
                if (xoff[s] < 0 || ctx->sn_owner[s] != me) continue;
                const Supernode &S = F.sn[s]; const int fc = S.ncols + S.nrows;
                PackTask T{}; T.U = front(s) + S.ncols + (size_t)fc * S.ncols; T.out = d_xbuf + xoff[s]; T.rc = S.nrows; T.fc = fc;
                pack.push_back(T); gx = std::max(gx, (S.nrows + 7) / 8);
            }
            if (!pack.empty()) launches.push_back({3, 0, (int)pack.size(), gx});
        }
        PH_CHK(hipMalloc(&d_gemm, sizeof(GemmTask) * std::max<size_t>(gemm.size(), 1)));
        PH_CHK(hipMalloc(&d_potrf, sizeof(PotrfTask) * std::max<size_t>(potrf.size(), 1)));
        PH_CHK(hipMalloc(&d_ext, sizeof(ExtendTask) * std::max<size_t>(ext.size(), 1)));
        PH_CHK(hipMalloc(&d_pack, sizeof(PackTask) * std::max<size_t>(pack.size(), 1)));
        PH_CHK(hipMemcpyAsync(d_gemm, gemm.data(), sizeof(GemmTask) * gemm.size(), hipMemcpyHostToDevice, st));
        PH_CHK(hipMemcpyAsync(d_potrf, potrf.data(), sizeof(PotrfTask) * potrf.size(), hipMemcpyHostToDevice, st));
        PH_CHK(hipMemcpyAsync(d_ext, ext.data(), sizeof(ExtendTask) * ext.size(), hipMemcpyHostToDevice, st));
        PH_CHK(hipMemcpyAsync(d_pack, pack.data(), sizeof(PackTask) * pack.size(), hipMemcpyHostToDevice, st));
        PH_CHK(hipStreamSynchronize(st));
        const double tk = now_s();
        if (verbose) fprintf(stderr, "admm_hip: factorization phase: scatter map of A %.3f s, fronts (malloc + clear) / task records / uploads %.3f s\n", t_maps, tk - tp - t_maps);
        hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, nnz, (const int64_t *)d_adst, (const int *)d_asrc, (const double *)d_aval, d_fronts);
        constexpr int YMAX = 32768;
        for (const Launch &Lc : launches) {
            for (int off = 0; off < Lc.count; off += YMAX) {
                const int cnt = std::min(YMAX, Lc.count - off);
                if (Lc.kind == 0) hipLaunchKernelGGL(extend_add_kernel, dim3(Lc.gx, cnt), dim3(256), 0, st, (const ExtendTask *)(d_ext + Lc.first + off));
                else if (Lc.kind == 1) hipLaunchKernelGGL(potrf_inv_kernel, dim3(cnt), dim3(256), 0, st, (const PotrfTask *)(d_potrf + Lc.first + off), d_fail);
                else if (Lc.kind == 2) hipLaunchKernelGGL(gemm_f64_kernel, dim3(Lc.gx, cnt), dim3(256), 0, st, (const GemmTask *)(d_gemm + Lc.first + off));
                else hipLaunchKernelGGL(pack_lower_kernel, dim3(Lc.gx, cnt), dim3(256), 0, st, (const PackTask *)(d_pack + Lc.first + off));
            }
        }
        PH_CHK(hipGetLastError());
        PH_CHK(hipStreamSynchronize(st));      // (the fronts and task records go before the next phase's arrive)
#undef PH_CHK
        const double tk1 = now_s();
        pfree();
        t_kernels += tk1 - tk;
        if (verbose) fprintf(stderr, "admm_hip: factorization phase: kernels %.3f s, freeing the fronts %.3f s\n", tk1 - tk, now_s() - tk1);
        n_launches += launches.size(); n_gemm += gemm.size(); n_potrf += potrf.size(); n_ext += ext.size();
        if (verbose) {
            for (const GemmTask &T : gemm) {      // products as issued (triangular operands are multiplied as dense blocks from their first non-zero block on)
                const int tm = (T.m + 63) / 64, tn = (T.n + 63) / 64;
                for (int ti = 0; ti < tm; ++ti) for (int tj = 0; tj < tn; ++tj) {
                    if ((T.flags & GEMM_LOWER_TILES) && tj > ti) continue;
                    const int k0 = (T.flags & GEMM_K_FROM_COL) ? 64 * tj : ((T.flags & GEMM_K_FROM_MAX) ? 64 * std::max(ti, tj) : 0);
                    flop += 2.0 * std::min(64, T.m - 64 * ti) * std::min(64, T.n - 64 * tj) * std::max(0, T.k - k0);
                }
            }
            if (local) fprintf(stderr, "admm_hip: rank %d: %s: fronts %.2f GB, %.3f s\n", me, pack_roots ? "own subtrees" : "replicated top", ftot * 8e-9, now_s() - tp);
        }
        return ADMM_OK;
    };

    double t_exchange = 0.0;
    int rc = ADMM_OK, failed = 0;
    if (!local) {
        rc = phase([](int) { return true; }, ftot_own, false);
        if (rc) { cleanup(); return rc; }
        DF_CHK(hipMemcpyAsync(&failed, d_fail, sizeof(int), hipMemcpyDeviceToHost, st));
        DF_CHK(hipStreamSynchronize(st));
    } else {
        // From here on every rank reaches both collectives whatever happens on it: a rank that returned early would leave the others
        // waiting in the exchange or in the consensus.  A rank whose own phase failed contributes what its buffer holds and skips the top.
        {
            std::lock_guard<std::mutex> one_rank_at_a_time(g_own_fronts_mutex);
            rc = phase(is_mine, ftot_own, true);
        }
        if (xtot) {      // the ONE collective of this factorization
            const double tx = now_s();
            // (in pieces of at most 2^27 doubles = 1 GB: a host-staged transport allocates its pinned buffer by the largest call)
            for (int64_t off = 0; off < xtot; off += (int64_t)1 << 27) {
                const int xrc = do_allreduce(ctx, d_xbuf + off, std::min<int64_t>((int64_t)1 << 27, xtot - off));
                if (!rc) rc = xrc;
            }
            if (!rc && verbose) { (void)hipStreamSynchronize(st); t_exchange = now_s() - tx; }
        }
        if (!rc) {      // (distributed top: the root's front and L^-1 are k^2 doubles each -- contexts sharing a device take turns here too)
            std::unique_lock<std::mutex> one_rank_at_a_time(g_own_fronts_mutex, std::defer_lock);
            if (ctx->dist_top) one_rank_at_a_time.lock();
            rc = phase(is_top, ftot_top, false);
        }
        if (!rc && (hipMemcpyAsync(&failed, d_fail, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
            rc = fail(ctx, ADMM_ERR_HIP, "device factorization: reading the pivot flag failed");
        // the consensus: every rank's outcome (-error code, or the first failing supernode + 1, or 0) in its own slot of ONE all-reduce of `world`
        // doubles.  Every rank then returns the same: the error of the lowest rank that had one (a rank keeps an error of its own), else
        // ADMM_ERR_FACTOR naming the lowest-numbered failing supernode -- a descendant's number is lower than its ancestors', so that is the
        // failure no other one caused (what the host factorization reports)
        std::vector<double> outcome(world, 0.0);
        outcome[me] = rc ? -(double)rc : (double)failed;
        int crc = hipMemcpyAsync(d_cons + 1, outcome.data(), sizeof(double) * world, hipMemcpyHostToDevice, st) == hipSuccess ? ADMM_OK : ADMM_ERR_HIP;
        { const int arc = do_allreduce(ctx, d_cons + 1, world); if (!crc) crc = arc; }
        if (!crc && (hipMemcpyAsync(outcome.data(), d_cons + 1, sizeof(double) * world, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) crc = ADMM_ERR_HIP;
        if (crc && !rc) rc = crc == ADMM_ERR_HIP ? fail(ctx, ADMM_ERR_HIP, "device factorization: the outcome consensus failed") : crc;
        if (!crc) {
            int bad_rank = -1; failed = 0;
            for (int r = 0; r < world; ++r) {
                if (outcome[r] < 0.0) { if (bad_rank < 0) bad_rank = r; }
                else if (outcome[r] > 0.0) failed = failed ? std::min(failed, (int)outcome[r]) : (int)outcome[r];
            }
            if (bad_rank >= 0 && !rc) rc = fail(ctx, (int)-outcome[bad_rank], "device factorization failed on rank %d of %d (error %d)", bad_rank, world, (int)-outcome[bad_rank]);
        }
        if (rc) { cleanup(); return rc; }
    }
#undef DF_CHK
    cleanup();
    F.panels.clear(); F.panels.shrink_to_fit();
    ctx->info.t_numeric_s = now_s() - t0;
    ctx->info.device_factor = 1;
    ctx->info.front_doubles = std::max(ftot_own, ftot_top); ctx->info.factor_exchange_doubles = xtot;
    if (verbose) {
        fprintf(stderr, "admm_hip: numeric factorization on the device%s: %.3f s, of which %.3f s of kernels (%.1f GFLOP in products: %.1f TFLOP/s) -- the rest is host set-up (maps, task records, uploads)%s; "
                        "fronts %.2f GB, %zu launches, %zu gemm / %zu potrf / %zu extend-add tasks\n", local ? " (rank-local)" : "",
                ctx->info.t_numeric_s, t_kernels, flop * 1e-9, flop / std::max(t_kernels, 1e-9) * 1e-12, local ? " and the exchange" : "", std::max(ftot_own, ftot_top) * 8e-9, n_launches, n_gemm, n_potrf, n_ext);
        if (local) fprintf(stderr, "admm_hip: rank %d: exchanged the subtree roots' update matrices: %.1f MB in one all-reduce, %.3f s (incl. the wait for the slowest rank)\n", me, xtot * 8e-6, t_exchange);
    }
    if (failed) return fail(ctx, ADMM_ERR_FACTOR, "system matrix is not positive definite (supernode %d)", failed - 1);
    return ADMM_OK;
}

// the factor's panels into ctx->d_panels (allocated): computed on the device, or on the host and copied
int panels_to_device(admm_hip_ctx *ctx) {
    if (ctx->device_numeric) {
        const int rc = device_factorize(ctx);
        if (rc != ADMM_DEVFACTOR_NOFIT) return rc;
        fprintf(stderr, "admm_hip: the fronts do not fit the device memory that is free, factoring on the host\n");
        const int err = factorize(ctx->A, ctx->F, std::max(1, (int)ctx->info.host_threads));
        if (err) return fail(ctx, ADMM_ERR_FACTOR, "system matrix is not positive definite (supernode %d)", err - 1);
        ctx->info.t_numeric_s = ctx->F.t_numeric;
    }
    ctx->info.device_factor = 0;
    ctx->info.front_doubles = 0; ctx->info.factor_exchange_doubles = 0;
    const Factor &F = ctx->F;
    if (!ctx->factor_local_on) {
        HIPCHK(hipMemcpy(ctx->d_panels, F.panels.data(), F.panels.size() * sizeof(double), hipMemcpyHostToDevice));
        return ADMM_OK;
    }
    // rank-local layout, factor from the host (the whole one: the host path does not split): the resident supernodes' panels and inverses
    for (size_t s = 0; s < F.sn.size(); ++s) {
        const Supernode &S = F.sn[s];
        if (ctx->dev_panel_off[s] >= 0)
            HIPCHK(hipMemcpy(ctx->d_panels + ctx->dev_panel_off[s], F.panels.data() + S.panel_off, sizeof(double) * (size_t)(S.ncols + S.nrows) * S.ncols, hipMemcpyHostToDevice));
        if (ctx->dev_root_inv_off[s] >= 0) {
            const size_t ld = (size_t)root_inv_ld(S.ncols);
            const size_t r0 = (int)s == ctx->root_sn ? (size_t)ctx->root_r0 : 0, nr = (int)s == ctx->root_sn ? (size_t)(ctx->root_r1 - ctx->root_r0) : (size_t)S.ncols;      // (distributed top: this rank's rows)
            if (nr) HIPCHK(hipMemcpy(ctx->d_panels + ctx->dev_root_inv_off[s], F.panels.data() + S.root_inv_off + ld * r0, sizeof(double) * ld * nr, hipMemcpyHostToDevice));
        }
    }
    return ADMM_OK;
}
