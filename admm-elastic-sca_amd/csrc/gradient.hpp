// gradient.hpp -- g = dE_i/dd of the elements' energies of energy.hpp in the element's compact rows, and the tets' Cauchy stress;
// shared by the host (gradient_host.cpp: admm_hip_gradient_query, admm_hip_stress_query) and the device (kernels_gradient.hpp).  Both
// sides compile it with -ffp-contract=off and keep the operation order below, so they give the same bits.  Extension, no reference
// counterpart.
//
// d, s and the row layout are energy.hpp's (9 / 6 / 3 rows as mat_from_rows, d[6], d[9], d[3] read them).  The nodal internal force is
// f = -sum_i D_i^T g_i (kernels_gradient.hpp).
//
// Exact derivatives of the energy of energy.hpp:
//   TET_NH      s [mu d + (lambda L / 2 - mu) cof(d) / J],  cof = dJ/dd, L = admm_log(J J);  not finite where the energy is not
//   TET_STVK    s d S,  S = 2 mu E + lambda tr(E) I,  E = (d^T d - I) / 2
//   TRI_FUNG    k [u - (b u - c v) r | v - (a v - c u) r],  u, v = d's columns, a = |u|^2, b = |v|^2, c = u.v, g = a b - c c, r = (1/g)^2,
//               k = (s mu) admm_exp(I1 - 3)   (the chain rule through I1 = a + b + 1/g);  not finite where the energy is not
//   SPRING, BEND, ANCHOR   s (d - p) with the p of energy.hpp; an anchor: w^2 (x - t), a released one: 0
//   TET_LINEAR, TRI_STRAIN s (d - p), p the nearest rotation / isometry: the exact derivative of s/2 |d - p|^2 (p is the closest point
//               of a smooth manifold, so d - p is normal to it and dp/dd drops out)
// Projective force only -- NOT the derivative of the stored energy:
//   TET_VOLUME, TRI_AREA   s (d - p), p = project_tet_p<true> / project_triarea_p.  This is the force projective dynamics applies.  The
//               projections stop after 4 / `iters` Newton steps, so p is no closest point and central differences of energy.hpp differ
//               from s (d - p) by 2 % to 90 % (relative) where the limits are active.  Where they are inactive -- TET_VOLUME: 0 <= J and
//               lmin <= J <= lmax with J = det d; TRI_AREA: lmin <= sqrt(det(d^T d)) <= lmax, or iters <= 0 -- p is d itself and g is
//               returned as exactly 0, not as the rounding left by recomposing d from its SVD.
// Not finite: when any entry of g would not be finite, all of g is the canonical quiet NaN (fill_nan) -- the same bits on both sides,
// whatever sign a computed NaN would carry.  Such an element adds zeros to every sum and is counted (as n_infinite for energies).
//
// Tet stress (the four tet kinds): Cauchy sigma = (g d^T) / (V J), V the rest volume (Batch::measure), each off-diagonal pair
// symmetrised as (a + b) / 2; seven values xx, yy, zz, xy, xz, yz, von Mises = sqrt(1/2 [(xx-yy)^2 + (yy-zz)^2 + (zz-xx)^2] + 3 [xy^2 +
// xz^2 + yz^2]).  All seven are the canonical NaN where J <= 0, or J, g or a result is not finite.
//
// Operation order.  Sums of three are (a + b) + c, every product is rounded, as in energy.hpp; the rest is as written.
#pragma once
#include "energy.hpp"

namespace admm_gradient {

using admm_dev::Mat3;
using admm_energy::finite;
using admm_energy::sq3;

ADMM_HD double quiet_nan() { return __builtin_nan(""); }
template <int N> ADMM_HD bool all_finite(const double *g) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok & finite(g[i]);
    return ok;
}
template <int N> ADMM_HD void fill_nan(double *g) {
#pragma unroll
    for (int i = 0; i < N; ++i) g[i] = quiet_nan();
}
// -> is g finite?  (not: g becomes the canonical NaN)
template <int N> ADMM_HD bool seal(double *g) {
    const bool ok = all_finite<N>(g);
    if (!ok) fill_nan<N>(g);
    return ok;
}
ADMM_HD void rows_from_mat(const Mat3 &m, double *g) {      // (the inverse of admm_energy::mat_from_rows)
    g[0] = m.m00; g[1] = m.m10; g[2] = m.m20; g[3] = m.m01; g[4] = m.m11; g[5] = m.m21; g[6] = m.m02; g[7] = m.m12; g[8] = m.m22;
}

ADMM_HD void tet_nh(const Mat3 &d, double mu, double lambda, double s, double g[9]) {
    const double J = admm_dev::det3(d);
    const double L = admm_dev::admm_log(J * J);
    if (!(J > 0.0) || !finite(J) || !finite(L) || !finite(admm_energy::fro2(d))) { fill_nan<9>(g); return; }      // (where tet_nh's energy is +inf)
    const double q = ((0.5 * lambda) * L - mu) / J;
    Mat3 c;      // cof(d) = dJ/dd
    c.m00 = d.m11 * d.m22 - d.m12 * d.m21; c.m01 = d.m12 * d.m20 - d.m10 * d.m22; c.m02 = d.m10 * d.m21 - d.m11 * d.m20;
    c.m10 = d.m02 * d.m21 - d.m01 * d.m22; c.m11 = d.m00 * d.m22 - d.m02 * d.m20; c.m12 = d.m01 * d.m20 - d.m00 * d.m21;
    c.m20 = d.m01 * d.m12 - d.m02 * d.m11; c.m21 = d.m02 * d.m10 - d.m00 * d.m12; c.m22 = d.m00 * d.m11 - d.m01 * d.m10;
    Mat3 r;
    r.m00 = s * (mu * d.m00 + q * c.m00); r.m10 = s * (mu * d.m10 + q * c.m10); r.m20 = s * (mu * d.m20 + q * c.m20);
    r.m01 = s * (mu * d.m01 + q * c.m01); r.m11 = s * (mu * d.m11 + q * c.m11); r.m21 = s * (mu * d.m21 + q * c.m21);
    r.m02 = s * (mu * d.m02 + q * c.m02); r.m12 = s * (mu * d.m12 + q * c.m12); r.m22 = s * (mu * d.m22 + q * c.m22);
    rows_from_mat(r, g);
    seal<9>(g);
}

ADMM_HD void tet_stvk(const Mat3 &d, double mu, double lambda, double s, double g[9]) {
    // E as in admm_energy::tet_stvk
    const double c00 = sq3(d.m00, d.m10, d.m20), c11 = sq3(d.m01, d.m11, d.m21), c22 = sq3(d.m02, d.m12, d.m22);
    const double c01 = (d.m00 * d.m01 + d.m10 * d.m11) + d.m20 * d.m21;
    const double c02 = (d.m00 * d.m02 + d.m10 * d.m12) + d.m20 * d.m22;
    const double c12 = (d.m01 * d.m02 + d.m11 * d.m12) + d.m21 * d.m22;
    const double e00 = 0.5 * (c00 - 1.0), e11 = 0.5 * (c11 - 1.0), e22 = 0.5 * (c22 - 1.0);
    const double e01 = 0.5 * c01, e02 = 0.5 * c02, e12 = 0.5 * c12;
    const double lt = lambda * ((e00 + e11) + e22), m2 = 2.0 * mu;
    const double S00 = m2 * e00 + lt, S11 = m2 * e11 + lt, S22 = m2 * e22 + lt, S01 = m2 * e01, S02 = m2 * e02, S12 = m2 * e12;
    Mat3 r;      // s (d S), S symmetric
    r.m00 = s * ((d.m00 * S00 + d.m01 * S01) + d.m02 * S02); r.m10 = s * ((d.m10 * S00 + d.m11 * S01) + d.m12 * S02); r.m20 = s * ((d.m20 * S00 + d.m21 * S01) + d.m22 * S02);
    r.m01 = s * ((d.m00 * S01 + d.m01 * S11) + d.m02 * S12); r.m11 = s * ((d.m10 * S01 + d.m11 * S11) + d.m12 * S12); r.m21 = s * ((d.m20 * S01 + d.m21 * S11) + d.m22 * S12);
    r.m02 = s * ((d.m00 * S02 + d.m01 * S12) + d.m02 * S22); r.m12 = s * ((d.m10 * S02 + d.m11 * S12) + d.m12 * S22); r.m22 = s * ((d.m20 * S02 + d.m21 * S12) + d.m22 * S22);
    rows_from_mat(r, g);
    seal<9>(g);
}

template <bool VOLUME> ADMM_HD void tet_blend(const Mat3 &d, double lmin, double lmax, double s, double g[9]) {
    if (VOLUME) {      // limits inactive: p is d itself, g is exactly 0 (not the rounding of recomposing d from its SVD)
        const double J = admm_dev::det3(d);
        if (J >= 0.0 && J >= lmin && J <= lmax) {
#pragma unroll
            for (int i = 0; i < 9; ++i) g[i] = 0.0;
            return;
        }
    }
    const Mat3 p = admm_dev::project_tet_p<VOLUME>(d, lmin, lmax);
    Mat3 r;
    r.m00 = s * (d.m00 - p.m00); r.m10 = s * (d.m10 - p.m10); r.m20 = s * (d.m20 - p.m20);
    r.m01 = s * (d.m01 - p.m01); r.m11 = s * (d.m11 - p.m11); r.m21 = s * (d.m21 - p.m21);
    r.m02 = s * (d.m02 - p.m02); r.m12 = s * (d.m12 - p.m12); r.m22 = s * (d.m22 - p.m22);
    rows_from_mat(r, g);
    seal<9>(g);
}

ADMM_HD void tri_fung(const double d[6], double mu, double s, double g[6]) {
    const double a = sq3(d[0], d[1], d[2]), b = sq3(d[3], d[4], d[5]);
    const double c = (d[0] * d[3] + d[1] * d[4]) + d[2] * d[5];
    const double det = a * b - c * c;
    if (!(det > 0.0)) { fill_nan<6>(g); return; }
    const double ig = 1.0 / det;
    const double I1 = (a + b) + ig;
    const double ex = admm_dev::admm_exp(I1 - 3.0);
    if (!finite(ex - 1.0)) { fill_nan<6>(g); return; }      // (where tri_fung's energy is +inf)
    const double r = ig * ig, k = (s * mu) * ex;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double u = d[i], v = d[3 + i];
        g[i] = k * (u - (b * u - c * v) * r);
        g[3 + i] = k * (v - (a * v - c * u) * r);
    }
    seal<6>(g);
}
ADMM_HD void tri_strain(const double d[6], double s, double g[6]) {
    double U2[6], V[4], s0, s1;
    admm_dev::svd32(d, U2, s0, s1, V);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i + 3 * j] = s * (d[i + 3 * j] - (U2[i] * V[j] + U2[i + 3] * V[j + 2]));
    seal<6>(g);
}
ADMM_HD void tri_area(const double d[6], int iters, double lmin, double lmax, double s, double g[6]) {
    {      // limits inactive: p is d itself, g is exactly 0 (not the rounding of recomposing d from its SVD)
        const double a = sq3(d[0], d[1], d[2]), b = sq3(d[3], d[4], d[5]);
        const double c = (d[0] * d[3] + d[1] * d[4]) + d[2] * d[5];
        const double det = a * b - c * c, area = sqrt(det);
        if (iters <= 0 || (det >= 0.0 && area >= lmin && area <= lmax)) {
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = 0.0;
            return;
        }
    }
    double p[6];
    admm_dev::project_triarea_p(d, iters, lmin, lmax, p);
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = s * (d[i] - p[i]);
    seal<6>(g);
}

ADMM_HD void spring(const double d[3], double rest_length, double s, double g[3]) {
    const double nrm = sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double dn = d[j] / nrm;
        if (nrm <= 0.0) dn = 0.0;
        g[j] = s * (d[j] - rest_length * dn);
    }
    seal<3>(g);
}

ADMM_HD void bend(const double d[9], double a0, double a1, double a3, double s, double g[9]) {
    const double den = a0 * a0 + a3 * a3 + a1 * a1;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double d0 = d[j], d1 = d[3 + j], d2 = d[6 + j];
        const double lam = 2.0 * (a0 * d0 + a3 * d1 + a1 * d2) / den;
        const double p0 = d0 - 0.5 * a0 * lam, p1 = d1 - 0.5 * a3 * lam, p2 = d2 - 0.5 * a1 * lam;
        g[j] = s * (d0 - p0); g[3 + j] = s * (d1 - p1); g[6 + j] = s * (d2 - p2);
    }
    seal<9>(g);
}

ADMM_HD void anchor(const double x[3], const double t[3], double w2, bool active, double g[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] = active ? w2 * (x[j] - t[j]) : 0.0;
    seal<3>(g);
}

// one element from element-major data, arguments as admm_energy::element -> g [rows]
ADMM_HD void element(int kind, const double *d, const double *par, const double *rest, double s, double *g) {
    switch (kind) {
    case ADMM_KIND_TET_NH: tet_nh(admm_energy::mat_from_rows(d), par[0], par[1], s, g); break;
    case ADMM_KIND_TET_STVK: tet_stvk(admm_energy::mat_from_rows(d), par[0], par[1], s, g); break;
    case ADMM_KIND_TET_LINEAR: tet_blend<false>(admm_energy::mat_from_rows(d), 0.0, 0.0, s, g); break;
    case ADMM_KIND_TET_VOLUME: tet_blend<true>(admm_energy::mat_from_rows(d), par[1], par[2], s, g); break;
    case ADMM_KIND_TRI_FUNG: tri_fung(d, par[0], s, g); break;
    case ADMM_KIND_TRI_STRAIN: tri_strain(d, s, g); break;
    case ADMM_KIND_TRI_AREA: tri_area(d, (int)par[1], par[2], par[3], s, g); break;
    case ADMM_KIND_SPRING: spring(d, rest[0], s, g); break;
    case ADMM_KIND_BEND: bend(d, rest[0], rest[1], rest[3], s, g); break;
    case ADMM_KIND_ANCHOR: anchor(d, rest, s, par[1] != 0.0, g); break;
    }
}

ADMM_HD bool is_tet(int kind) { return kind >= ADMM_KIND_TET_LINEAR && kind <= ADMM_KIND_TET_STVK; }
// the scale s of a tet from its rest volume, with admm_lib::energy_scale's arithmetic
ADMM_HD double tet_scale(int kind, const double *par, double volume) {
    return (kind == ADMM_KIND_TET_NH || kind == ADMM_KIND_TET_STVK) ? volume : par[0] * volume;
}

// Cauchy stress of a tet from its rows d, its gradient g (rows) and its rest volume -> out[7]
ADMM_HD void tet_stress(const Mat3 &d, const double g[9], double volume, double out[7]) {
    const double J = admm_dev::det3(d);
    if (!(J > 0.0) || !finite(J) || !all_finite<9>(g)) { fill_nan<7>(out); return; }
    const double den = volume * J;
    // (g d^T)(i, j) = sum_c g(i, c) d(j, c), g(i, c) = g[3 c + i]
    const double dr[3][3] = {{d.m00, d.m01, d.m02}, {d.m10, d.m11, d.m12}, {d.m20, d.m21, d.m22}};      // dr[j][c]
    double t[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[i][j] = ((g[i] * dr[j][0] + g[3 + i] * dr[j][1]) + g[6 + i] * dr[j][2]) / den;
    out[0] = t[0][0]; out[1] = t[1][1]; out[2] = t[2][2];
    out[3] = 0.5 * (t[0][1] + t[1][0]); out[4] = 0.5 * (t[0][2] + t[2][0]); out[5] = 0.5 * (t[1][2] + t[2][1]);
    const double a = out[0] - out[1], b = out[1] - out[2], c = out[2] - out[0];
    out[6] = sqrt(0.5 * sq3(a, b, c) + 3.0 * sq3(out[3], out[4], out[5]));
    seal<7>(out);
}

} // namespace admm_gradient
