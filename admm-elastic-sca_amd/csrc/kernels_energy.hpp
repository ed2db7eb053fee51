// kernels_energy.hpp -- the energies of energy.hpp evaluated on the device, and their sums.  Extension, no reference counterpart; no
// product path launches any of this unless the caller asks (admm_hip_energy, admm_hip_batch_energy[_dx], admm_hip_enable_objective).
//
// Per-element kernels, one per family (tets, triangles, hinges, springs, anchors): one lane per element, 64-element blocks of their
// own -- independent of the local step's block size, launch mode, cost order and pre-reduction.  The loads are the local step's (SoA,
// coalesced; the nodes' x gathered through idx), D_i x is formed by the local step's arithmetic (tets: tet_load_dx itself; the others:
// tri_load_dx, bend_load_dx, spring_load_dx, anchor_load_dx below, shared with the gradient kernels) and dx_override replaces it as it does there.  A lane beyond the batch returns before its first load.  Every lane writes E[e]; the
// block writes one partial, its lanes' values summed by the fixed butterfly of track_block_sum, where an element whose energy is not
// finite adds 0 to the partial and 1 to the block's count.
//
// Sums.  No atomics.  energy_reduce_kernel (one workgroup of 256 threads) combines n partials in an order that depends only on n:
// thread t adds partial[t], partial[t + 256], partial[t + 512], ... in ascending order, starting from 0.0; the 256 sums are then
// folded in LDS, acc[t] += acc[t + h] for h = 128, 64, ..., 1 with a barrier between the rounds; acc[0] is the total.  The counts go
// the same way as integers.  A batch's partials are one per 64 consecutive local elements, so its total depends on the batch's
// element count alone.
//
// Node terms, one lane per node in the CALLER's node order (iperm: caller's node -> device position), so that the sums do not depend
// on the elimination order (nor on how a run is sharded); 64-node blocks, the same partials and the same reduction:
//     kinetic  1/2 (((m0 v0) v0 + (m1 v1) v1) + (m2 v2) v2) per node
//     gravity  -(((m0 g0) x0 + (m1 g1) x1) + (m2 g2) x2) per node and constant explicit force g, over that force's nodes in its list's
//              order (all nodes: the caller's order); the partials of all forces are concatenated in list order and reduced at once
//     inertia  c (((m0 r0) r0 + (m1 r1) r1) + (m2 r2) r2), r_j = x_j - (M x_bar)_j / m_j, c = 1 / (2 dt^2)
//
// Cost: not measured, no timing claimed.  The element kernels hold no L-BFGS history and should be bound by memory: a tet reads its
// idx (16 B), four nodes' x (96 B), B (96 B), its parameters (8-24 B) and its scale (8 B) and writes 8 B.
#pragma once
#include "kernels_local.hpp"
#include "energy.hpp"

namespace admm_dev {

constexpr int ENERGY_BLOCK = 64;
constexpr int ENERGY_REDUCE = 256;
static_assert(ENERGY_BLOCK == 64, "the energy kernels' block sum is a 64-lane wave butterfly (track_block_sum)");

struct EnergyOut {
    const double *scale;   // [n]  the elements' scale s (energy.hpp)
    double *E;             // [n]  per-element energies
    double *partial;       // [blocks]
    int *n_inf;            // [blocks] elements of the block whose energy is not finite
};

__device__ __forceinline__ void energy_store(const EnergyOut &o, const int e, const double val) {
    o.E[e] = val;
    const bool bad = !admm_energy::finite(val);
    const unsigned long long act = __ballot(1), inf = __ballot(bad);
    track_block_sum(bad ? 0.0 : val, &o.partial[blockIdx.x]);
    if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)act) - 1)) o.n_inf[blockIdx.x] = __popcll(inf);
}

// KIND: ADMM_KIND_TET_LINEAR / _VOLUME / _NH / _STVK
template <int KIND>
__global__ __launch_bounds__(ENERGY_BLOCK) void energy_tet_kernel(BatchDev b, const double *__restrict__ x, EnergyOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double B[12]; Mat3 d;
    tet_load_dx(b, x, e, n, B, d);
    const double s = o.scale[e];
    double val;
    if (KIND == ADMM_KIND_TET_NH || KIND == ADMM_KIND_TET_STVK) {
        const double mu = b.par[(size_t)0 * n + e], lambda = b.par[(size_t)1 * n + e];
        val = KIND == ADMM_KIND_TET_NH ? admm_energy::tet_nh(d, mu, lambda, s) : admm_energy::tet_stvk(d, mu, lambda, s);
    } else if (KIND == ADMM_KIND_TET_VOLUME) {
        val = admm_energy::tet_blend<true>(d, b.par[(size_t)1 * n + e], b.par[(size_t)2 * n + e], s);
    } else val = admm_energy::tet_blend<false>(d, 0.0, 0.0, s);
    energy_store(o, e, val);
}

// The other families' inputs, as tet_load_dx gives the tets': the rest data that the energy and the gradient (kernels_gradient.hpp) both
// need and d = D_i x by the local step's arithmetic (project_tri_block, project_bend_block, project_spring_block, project_anchor_elem:
// their loads, their operation order), which dx_override then replaces.
__device__ __forceinline__ void tri_load_dx(const BatchDev &b, const double *__restrict__ x, int e, int n, double (&B)[6], double (&d)[6]) {
    const int4 id = reinterpret_cast<const int4 *>(b.idx)[e];
#pragma unroll
    for (int i = 0; i < 6; ++i) B[i] = b.rest[(size_t)i * n + e];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double xa = x[3 * (size_t)id.x + j], xb = x[3 * (size_t)id.y + j], xc = x[3 * (size_t)id.z + j];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            d[3 * r + j] = ((0.0 + B[0 + 3 * r] * xa) + B[1 + 3 * r] * xb) + B[2 + 3 * r] * xc;
            if (b.dx_override) d[3 * r + j] = b.dx_override[(size_t)(3 * r + j) * n + e];
        }
    }
}
// hinges: the rows x0 - x2, x3 - x2, x1 - x2
__device__ __forceinline__ void bend_load_dx(const BatchDev &b, const double *__restrict__ x, int e, int n, double &a0, double &a1, double &a3, double (&d)[9]) {
    const int4 id = reinterpret_cast<const int4 *>(b.idx)[e];
    a0 = b.rest[(size_t)0 * n + e]; a1 = b.rest[(size_t)1 * n + e]; a3 = b.rest[(size_t)3 * n + e];
    const int plus[3] = {id.x, id.w, id.y};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double x2 = x[3 * (size_t)id.z + j];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double xp = x[3 * (size_t)plus[r] + j];
            d[3 * r + j] = (plus[r] < id.z) ? ((0.0 + 1.0 * xp) + -1.0 * x2) : ((0.0 + -1.0 * x2) + 1.0 * xp);
            if (b.dx_override) d[3 * r + j] = b.dx_override[(size_t)(3 * r + j) * n + e];
        }
    }
}
// springs: the row x0 - x1
__device__ __forceinline__ void spring_load_dx(const BatchDev &b, const double *__restrict__ x, int e, int n, double &rest_length, double (&d)[3]) {
    const int ia = b.idx[2 * (size_t)e], ib = b.idx[2 * (size_t)e + 1];
    rest_length = b.rest[e];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double xa = x[3 * (size_t)ia + j], xb = x[3 * (size_t)ib + j];
        d[j] = (ia < ib) ? ((0.0 + 1.0 * xa) + -1.0 * xb) : ((0.0 + -1.0 * xb) + 1.0 * xa);
        if (b.dx_override) d[j] = b.dx_override[(size_t)j * n + e];
    }
}
// anchors: the node itself, its target (a released anchor: 0) and whether it is active
__device__ __forceinline__ void anchor_load_dx(const BatchDev &b, const double *__restrict__ x, int e, int n, double (&t)[3], bool &act, double (&d)[3]) {
    const int id = b.idx[e];
    act = b.active[e] != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d[j] = 0.0 + 1.0 * x[3 * (size_t)id + j];
        if (b.dx_override) d[j] = b.dx_override[(size_t)j * n + e];
        t[j] = act ? b.targets[3 * (size_t)e + j] : 0.0;
    }
}

// KIND: ADMM_KIND_TRI_STRAIN / _AREA / _FUNG
template <int KIND>
__global__ __launch_bounds__(ENERGY_BLOCK) void energy_tri_kernel(BatchDev b, const double *__restrict__ x, EnergyOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double B[6], d[6];
    tri_load_dx(b, x, e, n, B, d);
    const double s = o.scale[e];
    double val;
    if (KIND == ADMM_KIND_TRI_FUNG) val = admm_energy::tri_fung(d, b.par[e], s);
    else if (KIND == ADMM_KIND_TRI_AREA) val = admm_energy::tri_area(d, (int)b.par[(size_t)1 * n + e], b.par[(size_t)2 * n + e], b.par[(size_t)3 * n + e], s);
    else val = admm_energy::tri_strain(d, s);
    energy_store(o, e, val);
}

__global__ __launch_bounds__(ENERGY_BLOCK) void energy_bend_kernel(BatchDev b, const double *__restrict__ x, EnergyOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double a0, a1, a3, d[9];
    bend_load_dx(b, x, e, n, a0, a1, a3, d);
    energy_store(o, e, admm_energy::bend(d, a0, a1, a3, o.scale[e]));
}

__global__ __launch_bounds__(ENERGY_BLOCK) void energy_spring_kernel(BatchDev b, const double *__restrict__ x, EnergyOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double rest_length, d[3];
    spring_load_dx(b, x, e, n, rest_length, d);
    energy_store(o, e, admm_energy::spring(d, rest_length, o.scale[e]));
}

// an active anchor's distance from its target, weighted; a released one: 0
__global__ __launch_bounds__(ENERGY_BLOCK) void energy_anchor_kernel(BatchDev b, const double *__restrict__ x, EnergyOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double d[3], t[3]; bool act;
    anchor_load_dx(b, x, e, n, t, act, d);
    energy_store(o, e, admm_energy::anchor(d, t, b.w2[e], act));      // (the live weight^2: admm_hip_recompute_weights refreshes it)
}

// An element kernel of either output (EnergyOut here, GradOut in kernels_gradient.hpp) and each family's kernel, picked by the output's
// type: the one switch over the kinds (launch_element_kernel, abi_energy.inc) names the family and gets that output's kernel.
template <class Out> using ElementKernel = void (*)(BatchDev, const double *, Out);
template <int KIND> inline ElementKernel<EnergyOut> tet_kernel(const EnergyOut &) { return energy_tet_kernel<KIND>; }
template <int KIND> inline ElementKernel<EnergyOut> tri_kernel(const EnergyOut &) { return energy_tri_kernel<KIND>; }
inline ElementKernel<EnergyOut> bend_kernel(const EnergyOut &) { return energy_bend_kernel; }
inline ElementKernel<EnergyOut> spring_kernel(const EnergyOut &) { return energy_spring_kernel; }
inline ElementKernel<EnergyOut> anchor_kernel(const EnergyOut &) { return energy_anchor_kernel; }

// n partials (and, cnt != null, n counts) -> *total (and *count), in the fixed order described at the top.  One workgroup.
__global__ __launch_bounds__(ENERGY_REDUCE) void energy_reduce_kernel(const int n, const double *__restrict__ partial, const int *__restrict__ cnt,
                                                                      double *__restrict__ total, long long *__restrict__ count) {
    __shared__ double acc[ENERGY_REDUCE];
    __shared__ long long cacc[ENERGY_REDUCE];
    const int t = threadIdx.x;
    double a = 0.0; long long c = 0;
    for (int i = t; i < n; i += ENERGY_REDUCE) { a += partial[i]; if (cnt) c += cnt[i]; }
    acc[t] = a; cacc[t] = c;
    __syncthreads();
    for (int h = ENERGY_REDUCE / 2; h >= 1; h >>= 1) {
        if (t < h) { acc[t] += acc[t + h]; cacc[t] += cacc[t + h]; }
        __syncthreads();
    }
    if (t == 0) { *total = acc[0]; if (count) *count = cacc[0]; }
}

// TERM 0: kinetic (a = v, c = 1/2), 1: inertia (a = x, mxbar = M x_bar, c = 1 / (2 dt^2))
template <int TERM>
__global__ __launch_bounds__(ENERGY_BLOCK) void energy_node_kernel(const int n_nodes, const int *__restrict__ iperm, const double *__restrict__ m3, const double *__restrict__ a,
                                                                   const double *__restrict__ mxbar, const double c, double *__restrict__ partial) {
    const int i = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    const size_t p = 3 * (size_t)iperm[i];
    const double m0 = m3[p], m1 = m3[p + 1], m2 = m3[p + 2];
    double r0 = a[p], r1 = a[p + 1], r2 = a[p + 2];
    if (TERM == 1) { r0 = r0 - mxbar[p] / m0; r1 = r1 - mxbar[p + 1] / m1; r2 = r2 - mxbar[p + 2] / m2; }
    const double val = c * (((m0 * r0) * r0 + (m1 * r1) * r1) + (m2 * r2) * r2);
    track_block_sum(val, &partial[blockIdx.x]);
}

// one constant explicit force g over its nodes: idx (device positions, the list's order) or, idx == null, all nodes in the caller's order
__global__ __launch_bounds__(ENERGY_BLOCK) void energy_gravity_kernel(const int cnt, const int *__restrict__ idx, const int *__restrict__ iperm, const double *__restrict__ m3,
                                                                      const double *__restrict__ x, const double g0, const double g1, const double g2, double *__restrict__ partial) {
    const int i = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const size_t p = 3 * (size_t)(idx ? idx[i] : iperm[i]);
    const double val = -(((m3[p] * g0) * x[p] + (m3[p + 1] * g1) * x[p + 1]) + (m3[p + 2] * g2) * x[p + 2]);
    track_block_sum(val, &partial[blockIdx.x]);
}

} // namespace admm_dev
