// reaction.hpp -- the force a one-node constraint (COLLISION, ANCHOR: D_i = I on one node) exerted on its node in the last frame, its
// depth, the contact predicate and a contact's share of the resultant; shared by the host (reaction_host.cpp: admm_hip_reaction_query)
// and the device (kernels_reaction.hpp).  Both sides compile it with -ffp-contract=off and keep the operation order below, so they
// give the same bits.  Extension, no reference counterpart.
//
// A frame's last global solve satisfies   M (x - x_bar) / dt^2 = sum_i D_i^T w_i^2 (z_i - u_i - D_i x)   up to the linear solve's
// residual, with z_i, u_i what the last local step stored and x the final position.  Every collision form and the anchor kernel end
// with the same epilogue (u <- u + (dx - p), z <- p, slot = w^2 dt^2 (z - u): kernels_local.hpp), so for these two kinds element i's
// term is the force the constraint exerted on its node:
//     force    f_j = w2 * ((z_j - u_j) - x_j)                     three operations per component, in that order
//     depth    sqrt((u0 * u0 + u1 * u1) + u2 * u2)                five operations and the root; |u| is how far the constraint moved the node
//     contact  depth > depth_min                                  a NaN depth is no contact
//     torque   r = z - pivot;  (r1 f2 - r2 f1,  r2 f0 - r0 f2,  r0 f1 - r1 f0)       every product and difference rounded
// w2 is the element's weight^2 as the batch holds it (Batch::d_w2, filled for every built-in kind and refreshed by
// admm_hip_recompute_weights); nothing divides w^2 dt^2 by dt^2.
//
// The resultant's summation order (admm_hip_contact_resultant on the device, admm_hip_reaction_query on the host), per component of
// {sum f, sum torque} over the contacts k = 0, 1, ... in ascending order (node index / element index):
//   1. blocks of RESULTANT_BLOCK = 64 consecutive contacts, the last one padded with +0.0; a block's partial is the fold
//      a[i] = a[i] + a[i + h] for i < h, h = 32, 16, 8, 4, 2, 1; partial = a[0]   (track_block_sum's butterfly as lane 0 sees it)
//   2. the partials p[0 .. nb): acc[t] = ((0.0 + p[t]) + p[t + 256]) + p[t + 512] ... for t < RESULTANT_REDUCE = 256, then the fold
//      acc[t] = acc[t] + acc[t + h] for t < h, h = 128, 64, ..., 1; the total is acc[0]   (energy_reduce_kernel's order)
// Trailing +0.0 partials change no bit (a second-stage sum starts from +0.0 and so is never -0.0), so the device may reduce over more
// blocks than the contacts fill.
#pragma once
#include "local_math.hpp"

namespace admm_reaction {

constexpr int RESULTANT_BLOCK = 64, RESULTANT_REDUCE = 256;

ADMM_HD void force(const double w2, const double u[3], const double z[3], const double x[3], double f[3]) {
    f[0] = w2 * ((z[0] - u[0]) - x[0]);
    f[1] = w2 * ((z[1] - u[1]) - x[1]);
    f[2] = w2 * ((z[2] - u[2]) - x[2]);
}

ADMM_HD double depth(const double u[3]) { return sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]); }

ADMM_HD bool in_contact(const double depth, const double depth_min) { return depth > depth_min; }

// a contact's six terms of the resultant: its force, then the torque of that force at `point` about `pivot`
ADMM_HD void resultant_terms(const double f[3], const double point[3], const double pivot[3], double t[6]) {
    const double r0 = point[0] - pivot[0], r1 = point[1] - pivot[1], r2 = point[2] - pivot[2];
    t[0] = f[0]; t[1] = f[1]; t[2] = f[2];
    t[3] = r1 * f[2] - r2 * f[1];
    t[4] = r2 * f[0] - r0 * f[2];
    t[5] = r0 * f[1] - r1 * f[0];
}

} // namespace admm_reaction
