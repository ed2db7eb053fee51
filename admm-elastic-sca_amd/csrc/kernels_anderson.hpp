// kernels_anderson.hpp -- Anderson acceleration of the ADMM iteration (include/admm_hip.h), gfx950.
// Extension, no reference counterpart.
//
// The state s = (z, u) of all built-in batches is a list of segments (AASeg): a batch's z, then its u, each the batch's flat SoA
// array [rows][n_local] as the local step leaves it.  A segment of cnt doubles sits at the (even) offset `off` of every state-sized
// buffer: s_in, and the slots of the two rings (g and f = g - s_in, m + 1 slots of T doubles each).  Every elementwise kernel covers
// all segments in one launch, AA_PER_BLOCK doubles per 256-thread block; a block finds its segment by its number.
//
//   anderson_snapshot_kernel   s_in <- the batches' (z, u), before the local step
//   anderson_residual_kernel   after it: f = g - s_in, (g, f) -> the ring slot after the newest, and per block the partial sums of
//                              rho, of the newest difference's Gram row and of the right-hand side against the history's f
//   anderson_decide_kernel     one workgroup: sums the partials in an order that depends only on the block count, decides (accept /
//                              reset), advances the ring, keeps the differences' Gram matrix incrementally (never from a Gram of the
//                              columns: that cancels), solves for theta (anderson.hpp) and writes one log record
//   anderson_mix_kernel        reads the decision and theta from device memory: s_out = g - sum theta_j dG_j, or s_def, -> z, u
//   anderson_reslot_kernel, anderson_reslot_tet_kernel   the elements' right-hand-side shares dt^2 w^2 G^T (z - u) again from s_out
//                              (the projection kernels wrote them from g), in the slot layouts of kernels_local.hpp
// The mix and reslot kernels return at once when s_out = g (no history yet, the last iteration): the local step's own z, u and
// shares stand, bit for bit.  No atomics anywhere: a thread adds its elements in ascending order, a wave its lanes by a fixed
// butterfly, a block its four waves in order, the decide kernel the blocks like sum_partials_kernel.
//
// Memory traffic: every state-sized vector is streamed once per pass with 16-byte non-temporal loads and stores (read-once data;
// MI355X: 8-byte accesses reach 0.54-0.70 of the 16-byte rate).  Residual pass: g, s_in and min(entries, m) history f in, g and f
// out; mix pass: m_k + 1 history g in, z and u out.
#pragma once
#include <hip/hip_runtime.h>
#include "anderson.hpp"
#include "kernels_local.hpp"

namespace admm_dev {

constexpr int AA_BLOCK = 256, AA_PER_BLOCK = 1024, AA_MAX_M = admm_anderson::MAX_M, AA_RING_MAX = AA_MAX_M + 1, AA_NSUM = 1 + 2 * AA_MAX_M;
static_assert(AA_PER_BLOCK == 4 * AA_BLOCK, "two 16-byte pairs per thread");

struct AASeg {
    double *live;          // the batch's d_z or d_u
    const double *w2;      // [n_local] weight^2: element i of the segment belongs to local element i % n_local
    unsigned int n_local, cnt;      // cnt = rows * n_local
    int blk0, blk1;        // the segment's blocks [blk0, blk1)
    long long off;         // its (even) offset in every state-sized buffer
};

// the decision state, on the device only.  Ring slot of the newest entry `head`, entries `cnt` (0 .. m + 1); armed = 0: the next
// iteration is accepted whatever its rho (frame start -- the host zeroes the record -- and after a reset); def_slot: the ring slot whose
// g is s_def (the newest accepted entry: a rejected iteration writes the slot after it, never that one).
// action: 0 s_out = g (z, u stand as they are), 1 extrapolate, 2 reset.  ent[0 .. m_k]: the ring slots the mix reads, oldest first.
// gram: <dF_a, dF_b>_W indexed by the ring slots of the differences' newer entries.
struct AAState {
    int head, cnt, armed, def_slot;
    int action, m_k, pad0, pad1;
    int ent[AA_RING_MAX + 1];
    double rho_acc;
    double theta[AA_MAX_M];
    double gram[AA_RING_MAX * AA_RING_MAX];
};

typedef double aa_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ aa_v2 aa_ld2(const double *p) { return __builtin_nontemporal_load(reinterpret_cast<const aa_v2 *>(p)); }
__device__ __forceinline__ void aa_st2(double *p, aa_v2 v) { __builtin_nontemporal_store(v, reinterpret_cast<aa_v2 *>(p)); }
__device__ __forceinline__ double aa_ld1(const double *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void aa_st1(double *p, double v) { __builtin_nontemporal_store(v, p); }

__device__ __forceinline__ AASeg aa_find_seg(const AASeg *__restrict__ segs) {
    int s = 0;
    while ((int)blockIdx.x >= segs[s].blk1) ++s;      // (the grid has exactly the segments' blocks)
    return segs[s];
}
// first element of the thread's pair q (0, 1) in its block's part of the segment
__device__ __forceinline__ unsigned int aa_pair_first(const AASeg &sg, int q) {
    return (unsigned int)((int)blockIdx.x - sg.blk0) * AA_PER_BLOCK + 2u * (unsigned int)(q * AA_BLOCK + (int)threadIdx.x);
}

__global__ __launch_bounds__(AA_BLOCK) void anderson_snapshot_kernel(const AASeg *__restrict__ segs, double *__restrict__ s_in) {
    const AASeg sg = aa_find_seg(segs);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned int i = aa_pair_first(sg, q);
        if (i + 1 < sg.cnt) aa_st2(s_in + sg.off + i, aa_ld2(sg.live + i));
        else if (i < sg.cnt) aa_st1(s_in + sg.off + i, aa_ld1(sg.live + i));
    }
}

// partials [AA_NSUM][nblk]: 0 rho; with k = min(entries, m) >= 1 history entries h_0 (newest) .. h_k-1, d_new = f - f_h0 and
// d_j = f_hj - f_hj+1 (j = 0 .. k - 2):  1 <d_new, d_new>, 2 + j <d_new, d_j>,  1 + k <d_new, f>, 2 + k + j <d_j, f>; all weighted by w^2
__global__ __launch_bounds__(AA_BLOCK) void anderson_residual_kernel(const AASeg *__restrict__ segs, const AAState *__restrict__ st, int m, long long T,
                                                                       const double *__restrict__ s_in, double *__restrict__ ring_g, double *__restrict__ ring_f,
                                                                       int nblk, double *__restrict__ partials) {
    __shared__ double red[AA_BLOCK / 64][AA_NSUM];
    const AASeg sg = aa_find_seg(segs);
    const int head = st->head, cnt = st->cnt, R = m + 1;
    const int k = cnt < m ? cnt : m;
    const int w = cnt == 0 ? 0 : (head + 1) % R;
    double rho = 0.0, gr[AA_MAX_M], rh[AA_MAX_M];      // gr: <d_new, d_new>, <d_new, d_j>; rh: <d_new, f>, <d_j, f>
#pragma unroll
    for (int q = 0; q < AA_MAX_M; ++q) { gr[q] = 0.0; rh[q] = 0.0; }
    auto element = [&](double g, double si, const double (&fh)[AA_MAX_M], double w2, double &f) {
        f = g - si;
        rho += w2 * (f * f);
        if (k >= 1) {
            const double dn = f - fh[0];
            gr[0] += w2 * (dn * dn);
            rh[0] += w2 * (dn * f);
#pragma unroll
            for (int j = 0; j < AA_MAX_M - 1; ++j) if (j < k - 1) {
                const double dj = fh[j] - fh[j + 1];
                gr[1 + j] += w2 * (dn * dj);
                rh[1 + j] += w2 * (dj * f);
            }
        }
    };
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned int i = aa_pair_first(sg, q);
        const long long gi = sg.off + i;
        if (i + 1 < sg.cnt) {
            const aa_v2 g = aa_ld2(sg.live + i), si = aa_ld2(s_in + gi);
            double f0[AA_MAX_M], f1[AA_MAX_M];
#pragma unroll
            for (int j = 0; j < AA_MAX_M; ++j) {
                f0[j] = 0.0; f1[j] = 0.0;
                if (j < k) { const aa_v2 v = aa_ld2(ring_f + (long long)((head - j + R) % R) * T + gi); f0[j] = v.x; f1[j] = v.y; }
            }
            aa_v2 f;
            double fx, fy;
            element(g.x, si.x, f0, sg.w2[i % sg.n_local], fx);
            element(g.y, si.y, f1, sg.w2[(i + 1) % sg.n_local], fy);
            f.x = fx; f.y = fy;
            aa_st2(ring_g + (long long)w * T + gi, g);
            aa_st2(ring_f + (long long)w * T + gi, f);
        } else if (i < sg.cnt) {
            const double g = aa_ld1(sg.live + i), si = aa_ld1(s_in + gi);
            double f0[AA_MAX_M];
#pragma unroll
            for (int j = 0; j < AA_MAX_M; ++j) f0[j] = j < k ? aa_ld1(ring_f + (long long)((head - j + R) % R) * T + gi) : 0.0;
            double f;
            element(g, si, f0, sg.w2[i % sg.n_local], f);
            aa_st1(ring_g + (long long)w * T + gi, g);
            aa_st1(ring_f + (long long)w * T + gi, f);
        }
    }
    const int nq = 1 + 2 * k, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto wave_sum = [&](double a, int q) {      // a fixed butterfly over the wave's 64 lanes (all present)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) red[wave][q] = a;
    };
    wave_sum(rho, 0);
#pragma unroll
    for (int j = 0; j < AA_MAX_M; ++j) if (j < k) { wave_sum(gr[j], 1 + j); wave_sum(rh[j], 1 + k + j); }
    __syncthreads();
    if ((int)threadIdx.x < nq) {
        const int q = threadIdx.x;
        partials[(size_t)q * nblk + blockIdx.x] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

__global__ __launch_bounds__(AA_BLOCK) void anderson_decide_kernel(AAState *__restrict__ st, int m, int nblk, const double *__restrict__ partials, int last,
                                                                     admm_hip_acceleration_record *__restrict__ rec) {
    __shared__ double red[AA_BLOCK];
    __shared__ double sums[AA_NSUM];
    const int head = st->head, cnt = st->cnt, R = m + 1;
    const int k = cnt < m ? cnt : m;
    const int nq = 1 + 2 * k;
    for (int q = 0; q < nq; ++q) {      // (nq is uniform: every thread meets every barrier)
        double a = 0.0;
        for (int i = threadIdx.x; i < nblk; i += AA_BLOCK) a += partials[(size_t)q * nblk + i];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int off = AA_BLOCK / 2; off >= 1; off >>= 1) { if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off]; __syncthreads(); }
        if (threadIdx.x == 0) sums[q] = red[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    admm_hip_acceleration_record r;
    r.rho = sums[0]; r.accepted = 0; r.m_used = 0; r.extrapolated = 0; r.solve_failed = 0;
    for (int i = 0; i < 8; ++i) { r.theta[i] = 0.0; r.rhs[i] = 0.0; }
    for (int i = 0; i < 64; ++i) r.gram[i] = 0.0;
    const bool accept = st->armed == 0 || sums[0] < st->rho_acc;
    if (!accept) {      // reset: s_out = s_def, the history is emptied, the next iteration is accepted unconditionally
        st->action = 2; st->m_k = 0; st->cnt = 0; st->armed = 0;
        *rec = r;
        return;
    }
    const int w = cnt == 0 ? 0 : (head + 1) % R;
    if (k >= 1) {
        st->gram[w * AA_RING_MAX + w] = sums[1];
        for (int j = 0; j + 1 < k; ++j) { const int hj = (head - j + R) % R; st->gram[w * AA_RING_MAX + hj] = sums[2 + j]; st->gram[hj * AA_RING_MAX + w] = sums[2 + j]; }
    }
    st->head = w; st->cnt = cnt + 1 < R ? cnt + 1 : R; st->armed = 1; st->rho_acc = sums[0]; st->def_slot = w;
    const int mk = k;
    // the compact system, differences oldest first: a < mk - 1 is d_(k-2-a) (newer entry h_(k-2-a)), a = mk - 1 the newest difference
    int slot[AA_MAX_M];
    double b[AA_MAX_M], theta[AA_MAX_M];
    for (int a = 0; a < mk; ++a) {
        if (a == mk - 1) { slot[a] = w; b[a] = sums[1 + k]; }
        else { const int j = k - 2 - a; slot[a] = (head - j + R) % R; b[a] = sums[2 + k + j]; }
    }
    for (int a = 0; a < mk; ++a) { r.rhs[a] = b[a]; for (int c = 0; c < mk; ++c) r.gram[8 * a + c] = st->gram[slot[a] * AA_RING_MAX + slot[c]]; }
    int failed = 0;
    if (mk >= 1) failed = admm_anderson::solve(mk, r.gram, 8, b, theta);
    for (int a = 0; a < mk; ++a) { r.theta[a] = theta[a]; st->theta[a] = theta[a]; }
    for (int j = 0; j < k; ++j) st->ent[mk - 1 - j] = (head - j + R) % R;
    st->ent[mk] = w;
    const int extrapolate = mk >= 1 && !last && !failed;
    st->action = extrapolate; st->m_k = mk;
    r.accepted = 1; r.m_used = mk; r.extrapolated = extrapolate; r.solve_failed = failed;
    *rec = r;
}

// s_out = g - sum_j theta_j (g_ent[j+1] - g_ent[j]), j ascending (oldest difference first), every product rounded; or s_def
__global__ __launch_bounds__(AA_BLOCK) void anderson_mix_kernel(const AASeg *__restrict__ segs, const AAState *__restrict__ st, long long T, const double *__restrict__ ring_g) {
    const int action = st->action;
    if (action == 0) return;
    const AASeg sg = aa_find_seg(segs);
    if (action == 2) {
        const double *src = ring_g + (long long)st->def_slot * T + sg.off;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const unsigned int i = aa_pair_first(sg, q);
            if (i + 1 < sg.cnt) aa_st2(sg.live + i, aa_ld2(src + i));
            else if (i < sg.cnt) aa_st1(sg.live + i, aa_ld1(src + i));
        }
        return;
    }
    const int mk = st->m_k;
    double th[AA_MAX_M]; long long eo[AA_MAX_M + 1];
#pragma unroll
    for (int j = 0; j < AA_MAX_M; ++j) th[j] = j < mk ? st->theta[j] : 0.0;
#pragma unroll
    for (int j = 0; j <= AA_MAX_M; ++j) eo[j] = j <= mk ? (long long)st->ent[j] * T + sg.off : 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned int i = aa_pair_first(sg, q);
        if (i + 1 < sg.cnt) {
            aa_v2 prev = aa_ld2(ring_g + eo[0] + i), d[AA_MAX_M];      // (the sum of theta_j dG_j is not formed: the terms leave g one by one)
#pragma unroll
            for (int j = 0; j < AA_MAX_M; ++j) if (j < mk) { const aa_v2 nx = aa_ld2(ring_g + eo[j + 1] + i); d[j] = nx - prev; prev = nx; }
            aa_v2 a = prev;      // the newest g
#pragma unroll
            for (int j = 0; j < AA_MAX_M; ++j) if (j < mk) { a.x = a.x - th[j] * d[j].x; a.y = a.y - th[j] * d[j].y; }
            aa_st2(sg.live + i, a);
        } else if (i < sg.cnt) {
            double prev = aa_ld1(ring_g + eo[0] + i), d[AA_MAX_M];
#pragma unroll
            for (int j = 0; j < AA_MAX_M; ++j) if (j < mk) { const double nx = aa_ld1(ring_g + eo[j + 1] + i); d[j] = nx - prev; prev = nx; }
            double a = prev;
#pragma unroll
            for (int j = 0; j < AA_MAX_M; ++j) if (j < mk) a = a - th[j] * d[j];
            aa_st1(sg.live + i, a);
        }
    }
}

// the right-hand-side shares of a batch with one slot per corner, from the z, u the mix left: slot[dst[c]] = w2h2 * sum_r G[c][r] (z - u)[3r .. 3r+2]
// (residual_dual_kernel's shape; the projection kernels' own arithmetic up to the order of the scale)
__global__ __launch_bounds__(RES_BLOCK) void anderson_reslot_kernel(const AAState *__restrict__ st, int n, int nn, int cols, int ist, const double *__restrict__ z, const double *__restrict__ u,
                                                                      const double *__restrict__ w2h2, const double *__restrict__ G, const int *__restrict__ dst, double *__restrict__ slots) {
    if (st->action == 0) return;
    const int e = blockIdx.x * RES_BLOCK + threadIdx.x;
    if (e >= n) return;
    const double s = w2h2[e];
    double q[9];
    for (int i = 0; i < 3 * cols; ++i) q[i] = z[(size_t)i * n + e] - u[(size_t)i * n + e];
    for (int c = 0; c < nn; ++c) {
        double o0 = 0.0, o1 = 0.0, o2 = 0.0;
        for (int r = 0; r < cols; ++r) { const double g = G[(size_t)(3 * c + r) * n + e]; o0 += g * q[3 * r]; o1 += g * q[3 * r + 1]; o2 += g * q[3 * r + 2]; }
        double *o = slots + 3 * (size_t)dst[(size_t)ist * e + c];
        o[0] = s * o0; o[1] = s * o1; o[2] = s * o2;
    }
}

// ... of a tet batch with block-level pre-reduction (project_tet_block's epilogue: the block's corner shares summed per node in LDS in the
// staging order pos4 / bn_end, one slot per (block, node)); one wave per tpb-tet block
__global__ __launch_bounds__(LOCAL_BLOCK) void anderson_reslot_tet_kernel(const AAState *__restrict__ st, BatchDev b, const double *__restrict__ G) {
    __shared__ double stage[3 * 256];
    if (st->action == 0) return;
    const int blk = blockIdx.x, n = b.n;
    const int e = blk * b.tpb + threadIdx.x;
    if ((int)threadIdx.x >= b.tpb || e >= n) return;
    double q[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) q[i] = b.z[(size_t)i * n + e] - b.u[(size_t)i * n + e];
    const double s = b.w2h2[e];
    double f[12];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double g0 = G[(size_t)(3 * c) * n + e], g1 = G[(size_t)(3 * c + 1) * n + e], g2 = G[(size_t)(3 * c + 2) * n + e];
#pragma unroll
        for (int j = 0; j < 3; ++j) f[3 * c + j] = s * ((g0 * q[j] + g1 * q[3 + j]) + g2 * q[6 + j]);
    }
    const unsigned int p4 = b.pos4[e];
    const unsigned long long act = __ballot(1);
    const int nact = __popcll(act), lane = threadIdx.x & 63;
    const int q0 = b.bn_ptr[blk], q1 = b.bn_ptr[blk + 1];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int p = (p4 >> (8 * c)) & 255;
        stage[p] = f[3 * c]; stage[256 + p] = f[3 * c + 1]; stage[512 + p] = f[3 * c + 2];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // one wave per block: its own LDS writes are done, no barrier needed
    for (int i = q0 + lane; i < q1; i += nact) {
        const int k1 = b.bn_end[i], k0 = (i == q0) ? 0 : (int)b.bn_end[i - 1];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int kk = k0; kk < k1; ++kk) { a0 += stage[kk]; a1 += stage[256 + kk]; a2 += stage[512 + kk]; }
        double *o = b.fslot + 3 * (size_t)b.bn_dst[i];
        o[0] = a0; o[1] = a1; o[2] = a2;
    }
}

} // namespace admm_dev
