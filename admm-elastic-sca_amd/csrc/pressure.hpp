// pressure.hpp -- pressure chambers: a surface-normal load on an oriented triangle list, constant or by the isothermal gas law, added to
// v once per frame from the frame-start x; shared by the host (pressure_host.cpp: admm_hip_pressure_query; the checks of abi_pressure.inc)
// and the device (kernels_pressure.hpp).  Both sides compile it with -ffp-contract=off and keep the operation order below, so they give
// the same bits.  Extension, no reference counterpart.
//
// A chamber is an ordered list of oriented triangles (x0, x1, x2) over simulated nodes with a law.  Per frame, from the frame-start x:
//   per triangle   a = x1 - x0,  b = x2 - x0,  n = a x b;   r_k = x_k - o with o the position of the chamber's first triangle's first node;
//                  vol = (r0 . (r1 x r2)) / 6,   area = 0.5 sqrt(n . n)
//   per chamber    V = sum vol,  A = sum area,  N = sum 0.5 n   (five sums over the triangles in list order)
//   law            ADMM_PRESSURE_CONSTANT {p}: p as given (gauge);  ADMM_PRESSURE_GAS {amount, ambient}: p = amount / V - ambient, and
//                  p = 0 with `collapsed` counted when V is not > 0 or not finite;   resultant = p N
//   per node       f = sum over the node's corners of p_c n_t / 6 (for a closed fan exactly p grad_i V),  dv = (dt f) / m,  v <- v + dv
// o makes vol_t a difference of nearby points, so a chamber far from the origin loses no digits to its distance (a closed chamber's V
// does not depend on o).  A constant chamber with p == 0, or a gas chamber with amount == 0 and ambient == 0, is INACTIVE: the per-node
// gather passes over it, and a node in no active chamber is not written; its sums are still formed when its state is asked for.
//
// ORDER IN THE FRAME.  admm_hip_step adds the load after the body surfaces' update and the side latch and before gravity, the constant
// accelerations and the wind: pressure reads the frame-start surface the collision kernels see, and its increment is in v before gravity
// is added and before the wind reads v.
//
// Operation order.  Every product is rounded (no fused multiply-add).
//   cross(a, b) = (a1 b2 - a2 b1,  a2 b0 - a0 b2,  a0 b1 - a1 b0)                     (damping.hpp's)
//   dot(a, b)   = (a0 b0 + a1 b1) + a2 b2
//   vol  = dot(r0, cross(r1, r2)) / 6.0;   area = 0.5 * sqrt(dot(n, n));   N terms 0.5 * n_j
//   gas  p = amount / V - ambient
//   node f_j = ((0.0 + p_c g_j) + p_c' g'_j) + ...  with g_j = n_t[j] / 6.0, the node's corners ordered by chamber, then triangle, then
//        corner (a node CSR, node_csr.hpp), inactive chambers' corners left out;   dv_j = (dt * f_j) / m;   v_j = v_j + dv_j
// Summation order of V, A, N: damping.hpp's tree over the chamber's triangles k = 0, 1, ... in list order -- blocks of SUM_BLOCK = 64
// consecutive triangles, the last one padded with +0.0, folded a[i] = a[i] + a[i + h], h = 32 ... 1; then the partials through the
// SUM_REDUCE = 256 wide strided accumulate acc[t] = ((0.0 + p[t]) + p[t + 256]) + ... and the fold h = 128 ... 1.
#pragma once
#include <stdint.h>
#include <cmath>
#include <vector>
#include "local_math.hpp"
#include "damping.hpp"

namespace admm_pressure {

constexpr int SUM_BLOCK = admm_damping::SUM_BLOCK, SUM_REDUCE = admm_damping::SUM_REDUCE;
constexpr int N_SUMS = 5;                       // V, A, N[3]
constexpr int MODE_CONSTANT = 0, MODE_GAS = 1;  // = ADMM_PRESSURE_CONSTANT, ADMM_PRESSURE_GAS (include/admm_hip.h)

// = admm_hip_chamber_state (include/admm_hip.h)
struct Record {
    double volume, area, area_vector[3], pressure, resultant[3];
    int64_t n_tris, collapsed;
};

ADMM_HD double dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// a triangle's normal n = a x b and its five terms vol, area, 0.5 n
ADMM_HD void tri_terms(const double o[3], const double x0[3], const double x1[3], const double x2[3], double n[3], double t[N_SUMS]) {
    const double a[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, b[3] = {x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2]};
    admm_damping::cross(a, b, n);
    const double r0[3] = {x0[0] - o[0], x0[1] - o[1], x0[2] - o[2]}, r1[3] = {x1[0] - o[0], x1[1] - o[1], x1[2] - o[2]}, r2[3] = {x2[0] - o[0], x2[1] - o[1], x2[2] - o[2]};
    double c[3];
    admm_damping::cross(r1, r2, c);
    t[0] = dot(r0, c) / 6.0;
    t[1] = 0.5 * sqrt(dot(n, n));
    t[2] = 0.5 * n[0]; t[3] = 0.5 * n[1]; t[4] = 0.5 * n[2];
}

ADMM_HD bool active(const int mode, const double par0, const double par1) { return mode == MODE_GAS ? (par0 != 0.0 || par1 != 0.0) : par0 != 0.0; }

// the law: -> p; *collapsed = 1 where a gas chamber's volume is not > 0 or not finite (then p = 0)
ADMM_HD double law(const int mode, const double par0, const double par1, const double V, int *collapsed) {
    *collapsed = 0;
    if (mode != MODE_GAS) return par0;
    if (!(V > 0.0) || !(V <= 1.7976931348623157e308)) { *collapsed = 1; return 0.0; }
    return par0 / V - par1;
}

// the five sums -> the record's geometry, pressure and resultant (n_tris and collapsed are the caller's); returns the collapsed flag
ADMM_HD int finish(const double sum[N_SUMS], const int mode, const double par0, const double par1, Record &R) {
    R.volume = sum[0]; R.area = sum[1];
    R.area_vector[0] = sum[2]; R.area_vector[1] = sum[3]; R.area_vector[2] = sum[4];
    int collapsed;
    R.pressure = law(mode, par0, par1, sum[0], &collapsed);
    for (int j = 0; j < 3; ++j) R.resultant[j] = R.pressure * R.area_vector[j];
    return collapsed;
}

// one corner's share added to the node's force: f <- f + p (n / 6)
ADMM_HD void add_corner(const double p, const double n[3], double f[3]) {
    for (int j = 0; j < 3; ++j) f[j] = f[j] + p * (n[j] / 6.0);
}

// the node's increment dv = (dt f) / m
ADMM_HD void increment(const double dt, const double f[3], const double m, double dv[3]) {
    for (int j = 0; j < 3; ++j) dv[j] = (dt * f[j]) / m;
}

// ---- host side (never called from a kernel): the sums in the device's order, a chamber's record --------------------------------------
// the two-stage sum of damping.hpp over v[0 .. n)
inline double tree_sum(const std::vector<double> &v) {
    const size_t n = v.size(), nb = (n + SUM_BLOCK - 1) / SUM_BLOCK;
    std::vector<double> part(nb);
    for (size_t b = 0; b < nb; ++b) {
        double a[SUM_BLOCK];
        for (int i = 0; i < SUM_BLOCK; ++i) { const size_t k = b * SUM_BLOCK + i; a[i] = k < n ? v[k] : 0.0; }
        for (int h = SUM_BLOCK / 2; h >= 1; h >>= 1) for (int i = 0; i < h; ++i) a[i] = a[i] + a[i + h];
        part[b] = a[0];
    }
    double acc[SUM_REDUCE];
    for (int t = 0; t < SUM_REDUCE; ++t) { double s = 0.0; for (size_t i = t; i < nb; i += SUM_REDUCE) s += part[i]; acc[t] = s; }
    for (int h = SUM_REDUCE / 2; h >= 1; h >>= 1) for (int t = 0; t < h; ++t) acc[t] += acc[t + h];
    return acc[0];
}

// one chamber at the positions x [nodes][3] (the caller's ids in tris [nt][3]): its record (collapsed: this evaluation's flag) and,
// where nrm is given, the triangles' normals [nt][3]
inline void chamber_record(const double *x, const int32_t *tris, const int64_t nt, const int mode, const double par0, const double par1, Record &R, double *nrm) {
    std::vector<double> terms[N_SUMS];
    for (int q = 0; q < N_SUMS; ++q) terms[q].resize((size_t)nt);
    const double *o = x + 3 * (size_t)tris[0];
    for (int64_t t = 0; t < nt; ++t) {
        double n[3], s[N_SUMS];
        tri_terms(o, x + 3 * (size_t)tris[3 * t], x + 3 * (size_t)tris[3 * t + 1], x + 3 * (size_t)tris[3 * t + 2], n, s);
        for (int q = 0; q < N_SUMS; ++q) terms[q][(size_t)t] = s[q];
        if (nrm) { nrm[3 * t] = n[0]; nrm[3 * t + 1] = n[1]; nrm[3 * t + 2] = n[2]; }
    }
    double sum[N_SUMS];
    for (int q = 0; q < N_SUMS; ++q) sum[q] = tree_sum(terms[q]);
    R.n_tris = nt;
    R.collapsed = finish(sum, mode, par0, par1, R);
}

} // namespace admm_pressure
