// frame.hpp -- the rigid frame of a collision list entry and the analytic shapes' pushes, shared by the host (mesh.cpp:
// admm_hip_shape_query, admm_hip_mesh_query_framed) and the device (kernels_collision.hpp collide_analytic, project_collision_framed_kernel).
// Both sides compile it with -ffp-contract=off and keep the operation order below, so they give the same bits.  Extension, no reference
// counterpart beyond the three pushes themselves (CollisionFloor.hpp:51-58, CollisionSphere.hpp:50-66, CollisionCylinder.hpp:48-66).
//
// A frame is twelve doubles f = { R (3x3, row-major: R_jk = f[3j + k]), o = f[9..11] (pivot) }: the entry's shape, exactly as its params
// describe it, rotated by R about o.  The two maps, every product rounded, sums associated as written, no fused multiply-adds:
//     to_local   e = p - o;   q_j = o_j + (R_0j e_0 + (R_1j e_1 + R_2j e_2))          q = o + R^T (p - o)
//     to_world   e = q - o;   p_j = o_j + (R_j0 e_0 + (R_j1 e_1 + R_j2 e_2))          p = o + R (q - o)
//     rotate     v'_j = R_j0 v_0 + (R_j1 v_1 + R_j2 v_2)                              (a velocity given in the shape's own coordinates)
// A candidate goes to local coordinates, the entry's unframed code runs on it, and only a point that code moved goes back to world
// coordinates: a point the shape did not move keeps its bits.  identity(f) is R == I exactly (the pivot does not matter then, except to
// the box, whose centre it is): such an entry takes the unframed path.
#pragma once
#include <math.h>
#include "../../include/admm_kinds.h"

#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_frame {

ADMM_HD bool identity(const double *f) {
    return f[0] == 1.0 && f[1] == 0.0 && f[2] == 0.0 && f[3] == 0.0 && f[4] == 1.0 && f[5] == 0.0 && f[6] == 0.0 && f[7] == 0.0 && f[8] == 1.0;
}
ADMM_HD void to_local(const double *f, const double *p, double *q) {
    const double e0 = p[0] - f[9], e1 = p[1] - f[10], e2 = p[2] - f[11];
    q[0] = f[9] + (f[0] * e0 + (f[3] * e1 + f[6] * e2));
    q[1] = f[10] + (f[1] * e0 + (f[4] * e1 + f[7] * e2));
    q[2] = f[11] + (f[2] * e0 + (f[5] * e1 + f[8] * e2));
}
ADMM_HD void to_world(const double *f, const double *q, double *p) {
    const double e0 = q[0] - f[9], e1 = q[1] - f[10], e2 = q[2] - f[11];
    p[0] = f[9] + (f[0] * e0 + (f[1] * e1 + f[2] * e2));
    p[1] = f[10] + (f[3] * e0 + (f[4] * e1 + f[5] * e2));
    p[2] = f[11] + (f[6] * e0 + (f[7] * e1 + f[8] * e2));
}
ADMM_HD void rotate(const double *f, const double *v, double *o) {
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    o[0] = f[0] * v0 + (f[1] * v1 + f[2] * v2);
    o[1] = f[3] * v0 + (f[4] * v1 + f[5] * v2);
    o[2] = f[6] * v0 + (f[7] * v1 + f[8] * v2);
}

// floor y = c1, sphere (c, R), cylinder along z through (c0, c1) of radius R: p is pushed out when it is strictly inside; any other type
// does nothing (the box: collide_box; a mesh: mesh_query.hpp)
ADMM_HD void collide_round(const int ty, const double c0, const double c1, const double c2, const double R, double *p) {
    if (ty == ADMM_SHAPE_FLOOR) {
        if (c1 - p[1] > 0) p[1] = c1;
    } else if (ty == ADMM_SHAPE_SPHERE) {
        const double d0 = p[0] - c0, d1 = p[1] - c1, d2 = p[2] - c2;
        const double nrm = sqrt(d0 * d0 + (d1 * d1 + d2 * d2));
        if (R - nrm > 0) { p[0] = c0 + R * (d0 / nrm); p[1] = c1 + R * (d1 / nrm); p[2] = c2 + R * (d2 / nrm); }
    } else if (ty == ADMM_SHAPE_CYLINDER) {
        const double d0 = p[0] - c0, d1 = p[1] - c1, d2 = 0.0 - 0.0;
        const double nrm = sqrt(d0 * d0 + (d1 * d1 + d2 * d2));
        if (R - nrm > 0) { const double pz = p[2]; p[0] = (c0 + R * (d0 / nrm)) + 0.0; p[1] = (c1 + R * (d1 / nrm)) + 0.0; p[2] = (0.0 + R * (d2 / nrm)) + pz; }
    }
}

// the box of half extents h[3] centred at c[3], axes along the (local) coordinate axes:  d = p - c,  depth_j = h_j - |d_j|.  The point
// collides exactly when all three depths are > 0; it then moves to the face of least depth (ties: the lowest axis), to c_j + h_j when
// d_j >= 0 and to c_j - h_j otherwise, the other two coordinates untouched.  (No array indexed at run time: selects only.)
ADMM_HD void collide_box(const double *h, const double *c, double *p) {
    const double d0 = p[0] - c[0], d1 = p[1] - c[1], d2 = p[2] - c[2];
    const double g0 = h[0] - fabs(d0), g1 = h[1] - fabs(d1), g2 = h[2] - fabs(d2);
    if (!(g0 > 0 && g1 > 0 && g2 > 0)) return;
    if (g0 <= g1 && g0 <= g2) p[0] = d0 >= 0 ? c[0] + h[0] : c[0] - h[0];
    else if (g1 <= g2) p[1] = d1 >= 0 ? c[1] + h[1] : c[1] - h[1];
    else p[2] = d2 >= 0 ? c[2] + h[2] : c[2] - h[2];
}

// one analytic entry (type, par[4], frame f[12]; framed = !identity(f)) on the world-space candidate p -> did it move?  (the bits of p
// changed: what the kernel and admm_hip_shape_query both report)
ADMM_HD bool collide_entry(const int ty, const double *par, const double *f, const bool framed, double *p) {
    double q[3];
    if (framed) to_local(f, p, q); else { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
    const double b0 = q[0], b1 = q[1], b2 = q[2];
    if (ty == ADMM_SHAPE_BOX) collide_box(par, f + 9, q); else collide_round(ty, par[0], par[1], par[2], par[3], q);
    if (q[0] == b0 && q[1] == b1 && q[2] == b2) return false;
    if (framed) to_world(f, q, p); else { p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
    return true;
}

// host only: is f[12] a frame?  0: yes; 1: a value is not finite; 2: R is not a rotation (an element of R^T R - I, or det R - 1, beyond
// 1e-12 in size).  *which: the offending component of f (1), or 3 i + j of the first such element of R^T R - I, 9 for the determinant (2);
// *by: its value
inline int check(const double *f, int *which, double *by) {
    for (int k = 0; k < 12; ++k) if (!(fabs(f[k]) <= 1.79769313486231570815e308)) { *which = k; *by = f[k]; return 1; }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        const double g = (f[i] * f[j] + (f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j])) - (i == j ? 1.0 : 0.0);
        if (fabs(g) > 1e-12) { *which = 3 * i + j; *by = g; return 2; }
    }
    const double det = f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6]);
    if (fabs(det - 1.0) > 1e-12) { *which = 9; *by = det - 1.0; return 2; }
    return 0;
}

} // namespace admm_frame
