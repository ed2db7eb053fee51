// friction.hpp -- Coulomb friction at a collision contact, shared by the host (mesh.cpp: admm_hip_friction_query) and the device
// (kernels_collision.hpp project_collision_friction_kernel).  Both sides compile it with -ffp-contract=off and keep the operation order
// below, so they give the same bits.  Extension, no reference counterpart (the reference's contacts are frictionless).
//
// In a collision element the candidate is p = Dx + u, and at a resting contact u is the contact impulse over the weight: the depth by
// which a shape pushes p out to p' is the normal force, and the tangential part of p' - x0 (x0: the node at the start of the frame) is
// the tangential force plus the slip.  Clamping that tangential part against mu * depth is the Coulomb cone.  apply counts the obstacle
// as at rest; apply_moving takes the displacement w of the obstacle's surface over the frame at the contact (rigid_displacement for an
// entry's rigid motion, plus the interpolated vertex velocities of a mesh: mesh_query.hpp) and clamps the tangential part of
// (p' - x0) - w instead.  The result is not projected onto the shape again: on a curved surface it sits off the surface by
// O(|t|^2 / R), which the next ADMM iteration corrects.
#pragma once
#include <math.h>

#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_friction {

enum { NONE = 0, STICK = 1, SLIP = 2 };

// p: the point before the shape moved it, po: where the shape put it (in: p', out: p' after friction), x0: the node at the start of
// the frame, mu >= 0 (+inf: always sticks).  -> NONE (mu == 0 or the shape did not move the point: po untouched), STICK, SLIP
ADMM_HD int apply(const double *p, double *po, const double *x0, const double mu) {
    if (!(mu > 0.0)) return NONE;
    const double d0 = po[0] - p[0], d1 = po[1] - p[1], d2 = po[2] - p[2];
    const double depth = sqrt(d0 * d0 + (d1 * d1 + d2 * d2));
    if (depth == 0.0) return NONE;
    const double n0 = d0 / depth, n1 = d1 / depth, n2 = d2 / depth;
    const double r0 = po[0] - x0[0], r1 = po[1] - x0[1], r2 = po[2] - x0[2];
    const double rn = r0 * n0 + (r1 * n1 + r2 * n2);
    const double t0 = r0 - rn * n0, t1 = r1 - rn * n1, t2 = r2 - rn * n2;
    const double tl = sqrt(t0 * t0 + (t1 * t1 + t2 * t2));
    const double lim = mu * depth;
    if (tl <= lim) {      // stick: tangentially back where the frame started
        po[0] = po[0] - t0; po[1] = po[1] - t1; po[2] = po[2] - t2;
        return STICK;
    }
    const double s = lim / tl;      // slip: pulled back by the cone's radius
    po[0] = po[0] - s * t0; po[1] = po[1] - s * t1; po[2] = po[2] - s * t2;
    return SLIP;
}

// ... against a surface that moves: w[3] = the displacement of the obstacle's surface over the frame at the contact.  One line differs
// from apply, r = (po - x0) - w per component in that order; stick then means tangentially where the node would be had it ridden on
// the surface for the frame.  w = 0 gives the bits of apply.
ADMM_HD int apply_moving(const double *p, double *po, const double *x0, const double *w, const double mu) {
    if (!(mu > 0.0)) return NONE;
    const double d0 = po[0] - p[0], d1 = po[1] - p[1], d2 = po[2] - p[2];
    const double depth = sqrt(d0 * d0 + (d1 * d1 + d2 * d2));
    if (depth == 0.0) return NONE;
    const double n0 = d0 / depth, n1 = d1 / depth, n2 = d2 / depth;
    const double r0 = (po[0] - x0[0]) - w[0], r1 = (po[1] - x0[1]) - w[1], r2 = (po[2] - x0[2]) - w[2];
    const double rn = r0 * n0 + (r1 * n1 + r2 * n2);
    const double t0 = r0 - rn * n0, t1 = r1 - rn * n1, t2 = r2 - rn * n2;
    const double tl = sqrt(t0 * t0 + (t1 * t1 + t2 * t2));
    const double lim = mu * depth;
    if (tl <= lim) {      // stick: tangentially where the surface carried the frame's start
        po[0] = po[0] - t0; po[1] = po[1] - t1; po[2] = po[2] - t2;
        return STICK;
    }
    const double s = lim / tl;      // slip: pulled back by the cone's radius
    po[0] = po[0] - s * t0; po[1] = po[1] - s * t1; po[2] = po[2] - s * t2;
    return SLIP;
}

// the displacement over a frame of length dt, at the point c, of a surface in rigid motion m[9] = { a (linear velocity), om (angular
// velocity), o (pivot) }, world coordinates:  w = dt (a + om x (c - o)), in this order:
//     e = c - o;   x = (om1 e2 - om2 e1, om2 e0 - om0 e2, om0 e1 - om1 e0), each a difference of two products;   w_j = dt * (a_j + x_j)
ADMM_HD void rigid_displacement(const double *m, const double dt, const double *c, double *w) {
    const double e0 = c[0] - m[6], e1 = c[1] - m[7], e2 = c[2] - m[8];
    const double x0 = m[4] * e2 - m[5] * e1, x1 = m[5] * e0 - m[3] * e2, x2 = m[3] * e1 - m[4] * e0;
    w[0] = dt * (m[0] + x0); w[1] = dt * (m[1] + x1); w[2] = dt * (m[2] + x2);
}

} // namespace admm_friction
