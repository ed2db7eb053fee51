// damping.hpp -- velocity damping per node group, the filter applied to v after every frame; shared by the host (damping_host.cpp:
// admm_hip_damping_query) and the device (kernels_damping.hpp).  Both sides compile it with -ffp-contract=off and keep the operation
// order below, so they give the same bits.  Extension, no reference counterpart.
//
// A damping group is a range [node_first, node_first + node_count) of nodes in the caller's node order with two rates in 1/s,
// drag >= 0 (ether drag) and internal >= 0 (the momentum-preserving damping of Mueller et al., Position Based Dynamics, section 3.5:
// what is removed is the velocity that is NOT the group's rigid-body motion).  Per frame, on the state the epilogue left (x the new
// positions, v the new velocities), m_i the node's scalar mass:
//   pass 1   M = sum m_i,  S = sum m_i x_i,  P = sum m_i v_i,  T = sum 1/2 m_i |v_i|^2;   c = S / M,  v_c = P / M   (per component)
//   pass 2   r_i = x_i - c,  w_i = v_i - v_c:   L = sum m_i (r_i x w_i),   I = sum m_i (|r_i|^2 1 - r_i r_i^T), six entries xx yy zz xy xz yz
//   omega    = I^-1 L by the adjugate of the symmetric 3x3 matrix (solve_omega)
//   apply    beta = internal dt / (1 + internal dt),  s = 1 / (1 + drag dt), both formed once on the host (rates):
//            v_i <- v_i + beta ((v_c + omega x r_i) - v_i),   then   v_i <- s v_i
// A group with internal == 0 skips passes 1-2, omega and the first update: v_i <- s v_i alone.  A group with both rates zero is not
// touched.  A rigid motion is a fixed point of the first update, which changes neither P nor L about c.
//
// DEGENERATE GROUPS.  A group is degenerate when node_count < 3 or det I <= DAMPING_DEGENERATE (tr I / 3)^3 (a NaN counts as
// degenerate).  For a well-shaped body det I is about (tr I / 3)^3; DAMPING_DEGENERATE = 1e-10 refuses groups whose smallest principal
// moment is below about 1e-10 of the mean one -- all nodes on a line to five digits of the body's length -- where I^-1 L would be
// rounding noise.  A degenerate group gets omega = 0 and reports the flag: its target velocity is v_c alone, so ITS ROTATION IS DAMPED
// TOO (angular momentum is then not preserved).
//
// Operation order.  Every product is rounded.  Per node (node_terms_1, node_terms_2):
//   m x_j, m v_j;  1/2 m |v|^2 = 0.5 * (((m v0) v0 + (m v1) v1) + (m v2) v2)       (energy_node_kernel's kinetic term)
//   cross(a, b) = (a1 b2 - a2 b1,  a2 b0 - a0 b2,  a0 b1 - a1 b0);   L terms m * cross(r, w)_j
//   I terms  xx m * (r1 r1 + r2 r2),  yy m * (r0 r0 + r2 r2),  zz m * (r0 r0 + r1 r1),  xy -(m * (r0 r1)),  xz -(m * (r0 r2)),  yz -(m * (r1 r2))
// The adjugate and the determinant are written out in solve_omega; t_rigid = (0.5 M) ((vc0 vc0 + vc1 vc1) + vc2 vc2) +
// 0.5 ((om0 L0 + om1 L1) + om2 L2).
//
// Summation order of every sum above (no atomics; independent of the elimination order and of sharding), over the group's nodes
// k = 0, 1, ... in the caller's order counted from the group's first node:
//   1. blocks of SUM_BLOCK = 64 consecutive nodes, the last one padded with +0.0; a block's partial is the fold
//      a[i] = a[i] + a[i + h] for i < h, h = 32, 16, 8, 4, 2, 1; partial = a[0]   (track_block_sum's butterfly as lane 0 sees it)
//   2. the partials p[0 .. nb): acc[t] = ((0.0 + p[t]) + p[t + 256]) + p[t + 512] ... for t < SUM_REDUCE = 256, then the fold
//      acc[t] = acc[t] + acc[t + h] for t < h, h = 128, 64, ..., 1; the total is acc[0]   (energy_reduce_kernel's order)
#pragma once
#include <stdint.h>
#include "local_math.hpp"

namespace admm_damping {

constexpr int SUM_BLOCK = 64, SUM_REDUCE = 256;
constexpr int N_SUMS_1 = 8;       // pass 1: M, S[3], P[3], T
constexpr int N_SUMS_2 = 9;       // pass 2: L[3], I[6]
constexpr double DAMPING_DEGENERATE = 1e-10;

// = admm_hip_group_moments (include/admm_hip.h)
struct Moments {
    double mass, com[3], p[3], l[3], inertia[6], omega[3], t_total, t_rigid;
    int64_t n_nodes;
    int32_t degenerate, pad_;
};

// beta and s of the apply step from the rates and the time step (host side, once per frame and group)
ADMM_HD void rates(const double drag, const double internal, const double dt, double *beta, double *s) {
    *beta = (internal * dt) / (1.0 + internal * dt);
    *s = 1.0 / (1.0 + drag * dt);
}

ADMM_HD void cross(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a node's eight terms of pass 1
ADMM_HD void node_terms_1(const double m, const double x[3], const double v[3], double t[N_SUMS_1]) {
    t[0] = m;
    t[1] = m * x[0]; t[2] = m * x[1]; t[3] = m * x[2];
    t[4] = m * v[0]; t[5] = m * v[1]; t[6] = m * v[2];
    t[7] = 0.5 * (((m * v[0]) * v[0] + (m * v[1]) * v[1]) + (m * v[2]) * v[2]);
}

// pass 1's sums -> the record's mass, com, p, t_total and v_c
ADMM_HD void finish_1(const double sum[N_SUMS_1], Moments &R, double vc[3]) {
    R.mass = sum[0];
    for (int j = 0; j < 3; ++j) { R.com[j] = sum[1 + j] / sum[0]; R.p[j] = sum[4 + j]; vc[j] = sum[4 + j] / sum[0]; }
    R.t_total = sum[7];
}

// a node's nine terms of pass 2
ADMM_HD void node_terms_2(const double m, const double x[3], const double v[3], const double c[3], const double vc[3], double t[N_SUMS_2]) {
    const double r[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]}, w[3] = {v[0] - vc[0], v[1] - vc[1], v[2] - vc[2]};
    double rw[3];
    cross(r, w, rw);
    t[0] = m * rw[0]; t[1] = m * rw[1]; t[2] = m * rw[2];
    t[3] = m * (r[1] * r[1] + r[2] * r[2]);
    t[4] = m * (r[0] * r[0] + r[2] * r[2]);
    t[5] = m * (r[0] * r[0] + r[1] * r[1]);
    t[6] = -(m * (r[0] * r[1]));
    t[7] = -(m * (r[0] * r[2]));
    t[8] = -(m * (r[1] * r[2]));
}

// omega = I^-1 L, I = [xx xy xz; xy yy yz; xz yz zz] as inertia[6] = xx yy zz xy xz yz; returns the degenerate flag (then omega = 0)
ADMM_HD int solve_omega(const double I[6], const double L[3], const int64_t n_nodes, double om[3]) {
    const double xx = I[0], yy = I[1], zz = I[2], xy = I[3], xz = I[4], yz = I[5];
    const double a00 = yy * zz - yz * yz, a01 = xz * yz - xy * zz, a02 = xy * yz - xz * yy;
    const double a11 = xx * zz - xz * xz, a12 = xy * xz - xx * yz, a22 = xx * yy - xy * xy;
    const double det = (xx * a00 + xy * a01) + xz * a02;
    const double t3 = ((xx + yy) + zz) / 3.0;
    if (n_nodes < 3 || !(det > DAMPING_DEGENERATE * ((t3 * t3) * t3))) { om[0] = 0.0; om[1] = 0.0; om[2] = 0.0; return 1; }
    om[0] = ((a00 * L[0] + a01 * L[1]) + a02 * L[2]) / det;
    om[1] = ((a01 * L[0] + a11 * L[1]) + a12 * L[2]) / det;
    om[2] = ((a02 * L[0] + a12 * L[1]) + a22 * L[2]) / det;
    return 0;
}

// pass 2's sums -> the record's l, inertia, omega, t_rigid, degenerate (mass and n_nodes are already in it)
ADMM_HD void finish_2(const double sum[N_SUMS_2], const double vc[3], Moments &R) {
    for (int j = 0; j < 3; ++j) R.l[j] = sum[j];
    for (int j = 0; j < 6; ++j) R.inertia[j] = sum[3 + j];
    R.degenerate = solve_omega(R.inertia, R.l, R.n_nodes, R.omega);
    R.pad_ = 0;
    R.t_rigid = (0.5 * R.mass) * ((vc[0] * vc[0] + vc[1] * vc[1]) + vc[2] * vc[2]) + 0.5 * ((R.omega[0] * R.l[0] + R.omega[1] * R.l[1]) + R.omega[2] * R.l[2]);
}

// the internal update of one node's velocity: v <- v + beta ((v_c + omega x r) - v), r = x - c
ADMM_HD void apply_internal(const double beta, const double x[3], const double c[3], const double vc[3], const double om[3], double v[3]) {
    const double r[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]};
    double wr[3];
    cross(om, r, wr);
    for (int j = 0; j < 3; ++j) v[j] = v[j] + beta * ((vc[j] + wr[j]) - v[j]);
}

// ether drag: v <- s v
ADMM_HD void apply_drag(const double s, double v[3]) { v[0] = s * v[0]; v[1] = s * v[1]; v[2] = s * v[2]; }

} // namespace admm_damping
