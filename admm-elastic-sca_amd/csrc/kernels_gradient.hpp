// kernels_gradient.hpp -- the gradients of gradient.hpp evaluated on the device: per-element g = dE/dd, the corners' internal forces
// -D_i^T g, the tets' stress, and the nodes' sums.  Extension, no reference counterpart; no product path launches any of this unless the
// caller asks (admm_hip_batch_gradient[_dx], admm_hip_batch_stress, admm_hip_node_forces).
//
// Per-element kernels, one per family as in kernels_energy.hpp: one lane per element, ENERGY_BLOCK = 64-element blocks of their own --
// independent of the local step's block size, launch mode, cost order and pre-reduction.  The loads are the energy kernels' (the local
// step's: SoA, coalesced; the nodes' x gathered through idx), D_i x is formed by the local step's arithmetic (tet_load_dx and the energy
// kernels' tri_load_dx, bend_load_dx, spring_load_dx, anchor_load_dx themselves) and dx_override replaces it as it does there.  A lane beyond the batch returns before its first load.  Every lane writes
//     g   SoA [rows][n]
//     cf  SoA [3 nodes][n], cf[3 c + j] = component j of the force on stored corner c (the corner order of idx on the device):
//           tets       -((g[j] B(c, 0) + g[3 + j] B(c, 1)) + g[6 + j] B(c, 2))      B(c, r) = rest[c + 4 r]
//           triangles  -(g[j] B(c, 0) + g[3 + j] B(c, 1))                           B(c, r) = rest[c + 3 r]
//           hinges     node 0: -g[j], node 1: -g[6 + j], node 3: -g[3 + j], node 2: (g[j] + g[3 + j]) + g[6 + j]   (rows x0 - x2, x3 - x2, x1 - x2)
//           springs    node 0: -g[j], node 1: g[j]                                  (row x0 - x1)
//           anchors    -g[j]
//         all zeros for an element whose g is not finite: it adds nothing to a node's sum
//     stress SoA [7][n] (tets, when asked for)
// and the block writes the count of its elements whose g is not finite.
//
// Node gather, one lane per node in the CALLER's node order: the lane adds its incident corners' forces in the order of a CSR built on
// the host at first use -- batch order, then local element order, then the element's corners as the caller listed them -- by a
// compensated sequential sum: s = c = 0.0; per term v: t = s + v, bp = t - s, e = (s - (t - bp)) + (v - bp), s = t, c = c + e (Knuth's
// two_sum: t + e = s + v exactly); the result is s + c.  It is the exact sum rounded once, up to second order in 2^-53: the corner
// forces at a node cancel, and a plain sum errs by 2^-53 of their absolute sum, so that a rank's share and the one-rank vector would
// not agree to the last bits of their own size.  No atomics, no LDS: the sum depends on the scene alone, not on the elimination
// order, ADMM_HIP_TPB, ADMM_HIP_PRERED or the launch mode.
// The elastic batches and the anchor batches have a CSR each and go to two output vectors.  A node with no element gets exactly 0.0.
//
// Cost: not measured, no timing claimed.  Expected to be bound by memory: a tet reads what the energy kernel reads (232-248 B) and
// writes 72 B (g) + 96 B (cf) + 56 B (stress, when asked for); the gather reads a 12 B entry and 24 B per incident corner and writes 24 B per node.
#pragma once
#include "kernels_energy.hpp"
#include "gradient.hpp"

namespace admm_dev {

struct GradOut {
    const double *scale;   // [n]  the elements' scale s (energy.hpp)
    double *g;             // SoA [rows][n]
    double *cf;            // SoA [3 nodes][n]
    int *n_bad;            // [blocks] elements of the block whose g is not finite
    double *stress;        // tets: SoA [7][n], or NULL
    const double *volume;  // tets with stress: [n] rest volumes
};

__device__ __forceinline__ void gradient_count(const GradOut &o, const bool bad) {
    const unsigned long long act = __ballot(1), nb = __ballot(bad);
    if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)act) - 1)) o.n_bad[blockIdx.x] = __popcll(nb);
}

// KIND: ADMM_KIND_TET_LINEAR / _VOLUME / _NH / _STVK
template <int KIND>
__global__ __launch_bounds__(ENERGY_BLOCK) void gradient_tet_kernel(BatchDev b, const double *__restrict__ x, GradOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double B[12]; Mat3 d;
    tet_load_dx(b, x, e, n, B, d);
    const double s = o.scale[e];
    double g[9];
    if (KIND == ADMM_KIND_TET_NH || KIND == ADMM_KIND_TET_STVK) {
        const double mu = b.par[(size_t)0 * n + e], lambda = b.par[(size_t)1 * n + e];
        if (KIND == ADMM_KIND_TET_NH) admm_gradient::tet_nh(d, mu, lambda, s, g); else admm_gradient::tet_stvk(d, mu, lambda, s, g);
    } else if (KIND == ADMM_KIND_TET_VOLUME) {
        admm_gradient::tet_blend<true>(d, b.par[(size_t)1 * n + e], b.par[(size_t)2 * n + e], s, g);
    } else admm_gradient::tet_blend<false>(d, 0.0, 0.0, s, g);
    const bool ok = admm_gradient::all_finite<9>(g);
#pragma unroll
    for (int i = 0; i < 9; ++i) o.g[(size_t)i * n + e] = g[i];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.cf[(size_t)(3 * c + j) * n + e] = ok ? -((g[j] * B[c] + g[3 + j] * B[c + 4]) + g[6 + j] * B[c + 8]) : 0.0;
    if (o.stress) {
        double st[7];
        admm_gradient::tet_stress(d, g, o.volume[e], st);
#pragma unroll
        for (int i = 0; i < 7; ++i) o.stress[(size_t)i * n + e] = st[i];
    }
    gradient_count(o, !ok);
}

// KIND: ADMM_KIND_TRI_STRAIN / _AREA / _FUNG
template <int KIND>
__global__ __launch_bounds__(ENERGY_BLOCK) void gradient_tri_kernel(BatchDev b, const double *__restrict__ x, GradOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double B[6], d[6];
    tri_load_dx(b, x, e, n, B, d);
    const double s = o.scale[e];
    double g[6];
    if (KIND == ADMM_KIND_TRI_FUNG) admm_gradient::tri_fung(d, b.par[e], s, g);
    else if (KIND == ADMM_KIND_TRI_AREA) admm_gradient::tri_area(d, (int)b.par[(size_t)1 * n + e], b.par[(size_t)2 * n + e], b.par[(size_t)3 * n + e], s, g);
    else admm_gradient::tri_strain(d, s, g);
    const bool ok = admm_gradient::all_finite<6>(g);
#pragma unroll
    for (int i = 0; i < 6; ++i) o.g[(size_t)i * n + e] = g[i];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.cf[(size_t)(3 * c + j) * n + e] = ok ? -(g[j] * B[c] + g[3 + j] * B[c + 3]) : 0.0;
    gradient_count(o, !ok);
}

__global__ __launch_bounds__(ENERGY_BLOCK) void gradient_bend_kernel(BatchDev b, const double *__restrict__ x, GradOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double a0, a1, a3, d[9], g[9];
    bend_load_dx(b, x, e, n, a0, a1, a3, d);
    admm_gradient::bend(d, a0, a1, a3, o.scale[e], g);
    const bool ok = admm_gradient::all_finite<9>(g);
#pragma unroll
    for (int i = 0; i < 9; ++i) o.g[(size_t)i * n + e] = g[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.cf[(size_t)(0 + j) * n + e] = ok ? -g[j] : 0.0;
        o.cf[(size_t)(3 + j) * n + e] = ok ? -g[6 + j] : 0.0;
        o.cf[(size_t)(6 + j) * n + e] = ok ? (g[j] + g[3 + j]) + g[6 + j] : 0.0;
        o.cf[(size_t)(9 + j) * n + e] = ok ? -g[3 + j] : 0.0;
    }
    gradient_count(o, !ok);
}

__global__ __launch_bounds__(ENERGY_BLOCK) void gradient_spring_kernel(BatchDev b, const double *__restrict__ x, GradOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double rest_length, d[3], g[3];
    spring_load_dx(b, x, e, n, rest_length, d);
    admm_gradient::spring(d, rest_length, o.scale[e], g);
    const bool ok = admm_gradient::all_finite<3>(g);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.g[(size_t)j * n + e] = g[j];
        o.cf[(size_t)j * n + e] = ok ? -g[j] : 0.0;
        o.cf[(size_t)(3 + j) * n + e] = ok ? g[j] : 0.0;
    }
    gradient_count(o, !ok);
}

__global__ __launch_bounds__(ENERGY_BLOCK) void gradient_anchor_kernel(BatchDev b, const double *__restrict__ x, GradOut o) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x, n = b.n;
    if (e >= n) return;
    double d[3], t[3], g[3]; bool act;
    anchor_load_dx(b, x, e, n, t, act, d);
    admm_gradient::anchor(d, t, b.w2[e], act, g);      // (the live weight^2, as the energy kernel)
    const bool ok = admm_gradient::all_finite<3>(g);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.g[(size_t)j * n + e] = g[j];
        o.cf[(size_t)j * n + e] = ok ? -g[j] : 0.0;
    }
    gradient_count(o, !ok);
}

// the families' kernels of this output (kernels_energy.hpp: ElementKernel)
template <int KIND> inline ElementKernel<GradOut> tet_kernel(const GradOut &) { return gradient_tet_kernel<KIND>; }
template <int KIND> inline ElementKernel<GradOut> tri_kernel(const GradOut &) { return gradient_tri_kernel<KIND>; }
inline ElementKernel<GradOut> bend_kernel(const GradOut &) { return gradient_bend_kernel; }
inline ElementKernel<GradOut> spring_kernel(const GradOut &) { return gradient_spring_kernel; }
inline ElementKernel<GradOut> anchor_kernel(const GradOut &) { return gradient_anchor_kernel; }

// out[3 i + j] (caller's node i) = the compensated sum (above) of the node's incident corner forces in CSR order; entry k: component j at cf[off[k] + j stride[k]]
__global__ __launch_bounds__(ENERGY_BLOCK) void gradient_gather_kernel(const int n_nodes, const int *__restrict__ ptr, const long long *__restrict__ off, const int *__restrict__ stride,
                                                                       const double *__restrict__ cf, double *__restrict__ out) {
    const int i = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    double s[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
    for (int k = ptr[i], k1 = ptr[i + 1]; k < k1; ++k) {
        const double *p = cf + off[k];
        const size_t st = (size_t)stride[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) {      // two_sum: t + e = s + v exactly
            const double v = p[j * st], t = s[j] + v, bp = t - s[j], e = (s[j] - (t - bp)) + (v - bp);
            s[j] = t; c[j] = c[j] + e;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * (size_t)i + j] = s[j] + c[j];
}

} // namespace admm_dev
