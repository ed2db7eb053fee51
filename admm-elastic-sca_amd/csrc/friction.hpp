// friction.hpp -- Coulomb friction at a collision contact, shared by the host (mesh.cpp: admm_hip_friction_query) and the device
// (kernels_local.hpp project_collision_friction_kernel).  Both sides compile it with -ffp-contract=off and keep the operation order
// below, so they give the same bits.  Extension, no reference counterpart (the reference's contacts are frictionless).
//
// In a collision element the candidate is p = Dx + u, and at a resting contact u is the contact impulse over the weight: the depth by
// which a shape pushes p out to p' is the normal force, and the tangential part of p' - x0 (x0: the node at the start of the frame) is
// the tangential force plus the slip.  Clamping that tangential part against mu * depth is the Coulomb cone.  The obstacle counts as at
// rest (no velocity term), and the result is not projected onto the shape again: on a curved surface it sits off the surface by
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

} // namespace admm_friction
