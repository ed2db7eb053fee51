// energy.hpp -- the elements' energies E_i(D_i x) of the incremental potential
//     Phi(x) = 1 / (2 dt^2) |x - x_bar|^2_M + sum_i E_i(D_i x)
// shared by the host (energy_host.cpp: admm_hip_energy_query) and the device (kernels_energy.hpp).  Both sides compile it with
// -ffp-contract=off and keep the operation order below, so they give the same bits.  Extension, no reference counterpart (the
// reference never evaluates its objective).
//
// d = D_i x is the element's compact rows exactly as the local step forms them (kernels_local.hpp: tet_load, project_tri_block,
// project_bend_block, project_spring_block); the scaled dual variable u plays no part.  s is the element's scale
// (admm_hip_read_energy_scale): the rest volume / area for the hyperelastic kinds, kblend = stiffness * measure for the blended
// tets and triangles, the stiffness for springs and hinges.
//
//   TET_NH      s [mu/2 (I1 - L - 3) + lambda/8 L^2],  I1 = |d|^2_F, J = det d, L = admm_log(J J);  +inf when J <= 0 or not finite
//   TET_STVK    s [mu |E|^2_F + lambda/2 tr^2 E],  E = (d^T d - I) / 2;  finite for inverted elements too
//   TRI_FUNG    s mu/2 (admm_exp(I1 - 3) - 1),  I1 = |d|^2_F + 1/g, g = det(d^T d);  +inf when g <= 0 or the exponential overflows
//   TET_LINEAR, TET_VOLUME   s/2 |d - p|^2_F,  p = project_tet_p<VOLUME>(d, limits)
//   TRI_STRAIN  s/2 |d - T|^2,  T = U(:, :2) V^T of svd32(d)   (the strain limits are a hard clamp and carry no energy)
//   TRI_AREA    s/2 |d - p|^2,  p = project_triarea_p(d, iters, lmin, lmax)
//   SPRING      s/2 sum_j (d_j - p_j)^2,  p = L d / |d|, p = 0 where |d| <= 0
//   BEND        s/2 sum |d - p|^2,  p as in project_bend_block at u = 0
//   ANCHOR      active: w^2/2 |x - t|^2, released: 0   (a hard constraint in z: zero at convergence; reported apart from the elastic sum)
// The hyperelastic rows are Prox<TYPE>::value / FungProx::value at k = 0 written in invariants of d: no SVD.
//
// Operation order.  A sum of three squares is (a a + b b) + c c; a Frobenius norm adds its columns' sums in ascending column
// order, ((c0 + c1) + c2); every product is rounded.  The rest is as written in each function.
#pragma once
#include "local_math.hpp"
#include "../../include/admm_kinds.h"

namespace admm_energy {

using admm_dev::Mat3;

ADMM_HD double pos_inf() { return __builtin_inf(); }
ADMM_HD bool finite(double x) { return fabs(x) <= DBL_MAX; }
ADMM_HD double sq3(double a, double b, double c) { return (a * a + b * b) + c * c; }
ADMM_HD double fro2(const Mat3 &d) { return (sq3(d.m00, d.m10, d.m20) + sq3(d.m01, d.m11, d.m21)) + sq3(d.m02, d.m12, d.m22); }
ADMM_HD double dist2(const Mat3 &a, const Mat3 &b) {
    return (sq3(a.m00 - b.m00, a.m10 - b.m10, a.m20 - b.m20) + sq3(a.m01 - b.m01, a.m11 - b.m11, a.m21 - b.m21)) + sq3(a.m02 - b.m02, a.m12 - b.m12, a.m22 - b.m22);
}

ADMM_HD double tet_nh(const Mat3 &d, double mu, double lambda, double s) {
    const double J = admm_dev::det3(d);
    if (!(J > 0.0) || !finite(J)) return pos_inf();
    const double I1 = fro2(d);
    const double L = admm_dev::admm_log(J * J);
    if (!finite(L) || !finite(I1)) return pos_inf();      // J J under- or overflowed
    const double t1 = (0.5 * mu) * ((I1 - L) - 3.0);
    const double t2 = ((0.125 * lambda) * L) * L;
    return s * (t1 + t2);
}

ADMM_HD double tet_stvk(const Mat3 &d, double mu, double lambda, double s) {
    // C = d^T d, E = (C - I) / 2
    const double c00 = sq3(d.m00, d.m10, d.m20), c11 = sq3(d.m01, d.m11, d.m21), c22 = sq3(d.m02, d.m12, d.m22);
    const double c01 = (d.m00 * d.m01 + d.m10 * d.m11) + d.m20 * d.m21;
    const double c02 = (d.m00 * d.m02 + d.m10 * d.m12) + d.m20 * d.m22;
    const double c12 = (d.m01 * d.m02 + d.m11 * d.m12) + d.m21 * d.m22;
    const double e00 = 0.5 * (c00 - 1.0), e11 = 0.5 * (c11 - 1.0), e22 = 0.5 * (c22 - 1.0);
    const double e01 = 0.5 * c01, e02 = 0.5 * c02, e12 = 0.5 * c12;
    const double tr = (e00 + e11) + e22;
    const double ff = sq3(e00, e11, e22) + 2.0 * sq3(e01, e02, e12);
    return s * (mu * ff + (0.5 * lambda) * (tr * tr));
}

template <bool VOLUME> ADMM_HD double tet_blend(const Mat3 &d, double lmin, double lmax, double s) {
    const Mat3 p = admm_dev::project_tet_p<VOLUME>(d, lmin, lmax);
    return (0.5 * s) * dist2(d, p);
}

// triangles: d col-major 3x2
ADMM_HD double tri_fung(const double d[6], double mu, double s) {
    const double a = sq3(d[0], d[1], d[2]), b = sq3(d[3], d[4], d[5]);
    const double c = (d[0] * d[3] + d[1] * d[4]) + d[2] * d[5];
    const double g = a * b - c * c;
    if (!(g > 0.0)) return pos_inf();
    const double I1 = (a + b) + 1.0 / g;
    const double t = admm_dev::admm_exp(I1 - 3.0) - 1.0;
    if (!finite(t)) return pos_inf();
    return (s * (0.5 * mu)) * t;
}
ADMM_HD double dist2_6(const double d[6], const double p[6]) { return sq3(d[0] - p[0], d[1] - p[1], d[2] - p[2]) + sq3(d[3] - p[3], d[4] - p[4], d[5] - p[5]); }
ADMM_HD double tri_strain(const double d[6], double s) {
    double U2[6], V[4], s0, s1, T[6];
    admm_dev::svd32(d, U2, s0, s1, V);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) T[i + 3 * j] = U2[i] * V[j] + U2[i + 3] * V[j + 2];
    return (0.5 * s) * dist2_6(d, T);
}
ADMM_HD double tri_area(const double d[6], int iters, double lmin, double lmax, double s) {
    double p[6];
    admm_dev::project_triarea_p(d, iters, lmin, lmax, p);
    return (0.5 * s) * dist2_6(d, p);
}

ADMM_HD double spring(const double d[3], double rest_length, double s) {
    const double nrm = sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]));      // (project_spring_block's norm)
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double dn = d[j] / nrm;
        if (nrm <= 0.0) dn = 0.0;
        r[j] = d[j] - rest_length * dn;
    }
    return (0.5 * s) * sq3(r[0], r[1], r[2]);
}

// hinges: d[3 r + j], r = the row block (x0 - x2, x3 - x2, x1 - x2), j = the coordinate; a0, a3, a1 = alpha[0], alpha[3], alpha[1]
ADMM_HD double bend(const double d[9], double a0, double a1, double a3, double s) {
    const double den = a0 * a0 + a3 * a3 + a1 * a1;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double d0 = d[j], d1 = d[3 + j], d2 = d[6 + j];
        const double lam = 2.0 * (a0 * d0 + a3 * d1 + a1 * d2) / den;
        const double p0 = d0 - 0.5 * a0 * lam, p1 = d1 - 0.5 * a3 * lam, p2 = d2 - 0.5 * a1 * lam;
        acc = acc + sq3(d0 - p0, d1 - p1, d2 - p2);
    }
    return (0.5 * s) * acc;
}

ADMM_HD double anchor(const double x[3], const double t[3], double w2, bool active) {
    if (!active) return 0.0;
    return (0.5 * w2) * sq3(x[0] - t[0], x[1] - t[1], x[2] - t[2]);
}

ADMM_HD Mat3 mat_from_rows(const double *d) {      // rows of a tet element, element-major: column-major 3x3
    Mat3 m;
    m.m00 = d[0]; m.m10 = d[1]; m.m20 = d[2]; m.m01 = d[3]; m.m11 = d[4]; m.m21 = d[5]; m.m02 = d[6]; m.m12 = d[7]; m.m22 = d[8];
    return m;
}

// is the kind evaluated at all?  (collision and user-defined batches are not: value 0, counted as skipped)
ADMM_HD bool evaluated(int kind) { return kind >= 0 && kind < ADMM_KIND_COUNT && kind != ADMM_KIND_COLLISION; }

// one element from element-major data: d [rows], par [ADMM_KIND_PARAMS], rest [12] as admm_hip_read_rest lays it out (springs: the
// rest length in rest[0]; hinges: alpha[4]; anchors: the target in rest[0..2], par[1] != 0: active, s = weight^2; else unused)
ADMM_HD double element(int kind, const double *d, const double *par, const double *rest, double s) {
    switch (kind) {
    case ADMM_KIND_TET_NH: return tet_nh(mat_from_rows(d), par[0], par[1], s);
    case ADMM_KIND_TET_STVK: return tet_stvk(mat_from_rows(d), par[0], par[1], s);
    case ADMM_KIND_TET_LINEAR: return tet_blend<false>(mat_from_rows(d), 0.0, 0.0, s);
    case ADMM_KIND_TET_VOLUME: return tet_blend<true>(mat_from_rows(d), par[1], par[2], s);
    case ADMM_KIND_TRI_FUNG: return tri_fung(d, par[0], s);
    case ADMM_KIND_TRI_STRAIN: return tri_strain(d, s);
    case ADMM_KIND_TRI_AREA: return tri_area(d, (int)par[1], par[2], par[3], s);
    case ADMM_KIND_SPRING: return spring(d, rest[0], s);
    case ADMM_KIND_BEND: return bend(d, rest[0], rest[1], rest[3], s);
    case ADMM_KIND_ANCHOR: return anchor(d, rest, s, par[1] != 0.0);
    }
    return 0.0;
}

} // namespace admm_energy
