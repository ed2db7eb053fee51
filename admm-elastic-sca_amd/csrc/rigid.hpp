// rigid.hpp -- a rigid body in the collision list, moved by the reaction of its contacts; shared by the host (rigid_host.cpp:
// admm_hip_rigid_query; abi_rigid.inc: registration, admm_hip_set_rigid_state) and the device (kernels_rigid.hpp).  Both sides compile
// it with -ffp-contract=off and keep the operation order below, so they give the same bits.  Only + - * / and sqrt, no libm call.
// Extension, no reference counterpart.
//
// State of a body: c[3] the centre of mass, q[4] = (w, x, y, z) the orientation as a unit quaternion, v[3] the linear velocity, L[3]
// the angular momentum about c in world axes.  L is the state variable, omega is derived: a torque-free body keeps L exactly.
// Constants: mass, Jinv[6] = (xx, xy, xz, yy, yz, zz) the inverse of the inertia tensor about the centre of mass in the entry's own,
// unrotated coordinates (invert_inertia, at registration), accel[3], the registration values c0[3] and par0[4], the entry and its type.
//
// One frame (step), given the body's row (Fe, Te) of the entry sums about c -- what its contacts exerted ON THE NODES -- and dt.  Every
// product is rounded, sums are associated as written, no fused multiply-adds:
//   load       F_j = -Fe_j;  tau_j = -Te_j
//   velocity   v'_j = v_j + dt * (F_j / mass + accel_j)
//   momentum   L'_j = L_j + dt * tau_j
//   rotation   R = rotation(q):  with xx = x x, yy = y y, zz = z z, xy = x y, xz = x z, yz = y z, wx = w x, wy = w y, wz = w z
//                R00 = 1 - 2 (yy + zz)   R01 = 2 (xy - wz)       R02 = 2 (xz + wy)
//                R10 = 2 (xy + wz)       R11 = 1 - 2 (xx + zz)   R12 = 2 (yz - wx)
//                R20 = 2 (xz - wy)       R21 = 2 (yz + wx)       R22 = 1 - 2 (xx + yy)
//   omega      a_j = R_0j L'_0 + (R_1j L'_1 + R_2j L'_2)                           a = R^T L'
//              b_0 = J0 a_0 + (J1 a_1 + J2 a_2);  b_1 = J1 a_0 + (J3 a_1 + J4 a_2);  b_2 = J2 a_0 + (J4 a_1 + J5 a_2)       b = Jinv a
//              omega'_j = R_j0 b_0 + (R_j1 b_1 + R_j2 b_2)                         omega' = R b   (R is the rotation BEFORE this frame's turn)
//   centre     c'_j = c_j + dt * v'_j
//   turn       hd = dt / 2;  h_j = hd * omega'_j;  s = sqrt(1 + (h_0 h_0 + (h_1 h_1 + h_2 h_2)));  d = (1 / s, h_0 / s, h_1 / s, h_2 / s)
//              p = d (x) q, the Hamilton product with d on the left (a turn about world axes):
//                p_w = d_w q_w - (d_x q_x + (d_y q_y + d_z q_z))
//                p_x = d_w q_x + (d_x q_w + (d_y q_z - d_z q_y))
//                p_y = d_w q_y + (d_y q_w + (d_z q_x - d_x q_z))
//                p_z = d_w q_z + (d_z q_w + (d_x q_y - d_y q_x))
//              q' = p / sqrt(p_w p_w + (p_x p_x + (p_y p_y + p_z p_z)));   R' = rotation(q')
// d is the Cayley transform of h: an exact rotation about omega' by the angle 2 atan|h|, whatever the size of h.  That angle differs
// from dt |omega'| = 2 |h| by 2 (|h| - atan|h|) <= 2 |h|^3 / 3 = (dt |omega'|)^3 / 12 per frame.
//
// Pose written to the shape table (pose): frame' = { R', c' }, framed' = !admm_frame::identity(R'), motion' = { v', omega', c' } --
// what friction.hpp's rigid_displacement reads, so friction against the body uses the velocity that carried it to where it stands --
// and, for ADMM_SHAPE_SPHERE and ADMM_SHAPE_MESH, par'_j = par0_j + (c'_j - c0_j) for j < 3, par'_3 = par0_3; for ADMM_SHAPE_BOX
// par' = par0 (the box's centre is the frame's pivot).
#pragma once
#include <math.h>
#include <stdint.h>
#include "frame.hpp"

namespace admm_rigid {

struct Const { double mass, Jinv[6], accel[3], c0[3], par0[4]; int32_t entry, type; };
// = admm_hip_rigid_state (include/admm_hip.h): the state c, q, v, L; derived: omega, R (row-major), the entry's par; the last frame's
// applied F, tau and its number of contacts
struct Record { double c[3], q[4], v[3], L[3], omega[3], R[9], par[4], F[3], tau[3]; int64_t count; int32_t entry, pad_; };
static_assert(sizeof(Record) == 296, "the record is 35 doubles, a count and two ints");

ADMM_HD void rotation(const double *q, double *R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz); R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz); R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy); R[7] = 2.0 * (yz + wx); R[8] = 1.0 - 2.0 * (xx + yy);
}

// omega = R (Jinv (R^T L))
ADMM_HD void angular_velocity(const double *R, const double *J, const double *L, double *om) {
    const double a0 = R[0] * L[0] + (R[3] * L[1] + R[6] * L[2]);
    const double a1 = R[1] * L[0] + (R[4] * L[1] + R[7] * L[2]);
    const double a2 = R[2] * L[0] + (R[5] * L[1] + R[8] * L[2]);
    const double b0 = J[0] * a0 + (J[1] * a1 + J[2] * a2);
    const double b1 = J[1] * a0 + (J[3] * a1 + J[4] * a2);
    const double b2 = J[2] * a0 + (J[4] * a1 + J[5] * a2);
    om[0] = R[0] * b0 + (R[1] * b1 + R[2] * b2);
    om[1] = R[3] * b0 + (R[4] * b1 + R[5] * b2);
    om[2] = R[6] * b0 + (R[7] * b1 + R[8] * b2);
}

ADMM_HD void normalise(const double *p, double *q) {
    const double n = sqrt(p[0] * p[0] + (p[1] * p[1] + (p[2] * p[2] + p[3] * p[3])));
    q[0] = p[0] / n; q[1] = p[1] / n; q[2] = p[2] / n; q[3] = p[3] / n;
}

// q' = normalise(d (x) q), d the Cayley transform of h = (dt / 2) omega
ADMM_HD void turn(const double *q, const double *om, const double dt, double *qn) {
    const double hd = dt / 2.0;
    const double h0 = hd * om[0], h1 = hd * om[1], h2 = hd * om[2];
    const double s = sqrt(1.0 + (h0 * h0 + (h1 * h1 + h2 * h2)));
    const double dw = 1.0 / s, dx = h0 / s, dy = h1 / s, dz = h2 / s;
    double p[4];
    p[0] = dw * q[0] - (dx * q[1] + (dy * q[2] + dz * q[3]));
    p[1] = dw * q[1] + (dx * q[0] + (dy * q[3] - dz * q[2]));
    p[2] = dw * q[2] + (dy * q[0] + (dz * q[1] - dx * q[3]));
    p[3] = dw * q[3] + (dz * q[0] + (dx * q[2] - dy * q[1]));
    normalise(p, qn);
}

// the entry's par for the centre c
ADMM_HD void entry_par(const Const &K, const double *c, double *par) {
    const bool follows = K.type == ADMM_SHAPE_SPHERE || K.type == ADMM_SHAPE_MESH;
    for (int j = 0; j < 3; ++j) par[j] = follows ? K.par0[j] + (c[j] - K.c0[j]) : K.par0[j];
    par[3] = K.par0[3];
}

// one frame: S (its c, q, v, L are read) and the row (Fe, Te) about S.c -> every field of O.  O may be S.
ADMM_HD void step(const Const &K, const Record &S, const double *Fe, const double *Te, const int64_t count, const double dt, Record &O) {
    double F[3], tau[3], v[3], L[3], c[3], R[9], om[3], q[4];
    for (int j = 0; j < 3; ++j) { F[j] = -Fe[j]; tau[j] = -Te[j]; }
    for (int j = 0; j < 3; ++j) { v[j] = S.v[j] + dt * (F[j] / K.mass + K.accel[j]); L[j] = S.L[j] + dt * tau[j]; }
    rotation(S.q, R);
    angular_velocity(R, K.Jinv, L, om);
    for (int j = 0; j < 3; ++j) c[j] = S.c[j] + dt * v[j];
    turn(S.q, om, dt, q);
    for (int j = 0; j < 3; ++j) { O.c[j] = c[j]; O.v[j] = v[j]; O.L[j] = L[j]; O.omega[j] = om[j]; O.F[j] = F[j]; O.tau[j] = tau[j]; }
    for (int j = 0; j < 4; ++j) O.q[j] = q[j];
    rotation(q, O.R);
    entry_par(K, c, O.par);
    O.count = count; O.entry = K.entry; O.pad_ = 0;
}

// the derived fields of a state given from outside (registration, admm_hip_set_rigid_state): omega, R and par from c, q, L; no load yet
ADMM_HD void derive(const Const &K, Record &S) {
    rotation(S.q, S.R);
    angular_velocity(S.R, K.Jinv, S.L, S.omega);
    entry_par(K, S.c, S.par);
    for (int j = 0; j < 3; ++j) { S.F[j] = 0.0; S.tau[j] = 0.0; }
    S.count = 0; S.entry = K.entry; S.pad_ = 0;
}

// the body's rows of the shape table: par[4], frame[12], motion[9] -> framed
ADMM_HD int pose(const Record &S, double *par, double *frame, double *motion) {
    for (int j = 0; j < 4; ++j) par[j] = S.par[j];
    for (int k = 0; k < 9; ++k) frame[k] = S.R[k];
    for (int j = 0; j < 3; ++j) { frame[9 + j] = S.c[j]; motion[j] = S.v[j]; motion[3 + j] = S.omega[j]; motion[6 + j] = S.c[j]; }
    return admm_frame::identity(S.R) ? 0 : 1;
}

// ---- host only --------------------------------------------------------------------------------------------------------------------
// J[6] = (xx, xy, xz, yy, yz, zz) -> its inverse by cofactors; false: a value is not finite or J is not positive definite (Sylvester:
// xx > 0, the leading 2x2 minor > 0, det > 0).  Order: the six cofactors as differences of two products, det = xx C0 + (xy C1 + xz C2),
// every entry a cofactor divided by det.
inline bool invert_inertia(const double *J, double *Ji) {
    for (int k = 0; k < 6; ++k) if (!(fabs(J[k]) <= 1.79769313486231570815e308)) return false;
    const double a = J[0], b = J[1], c = J[2], d = J[3], e = J[4], f = J[5];
    const double C0 = d * f - e * e, C1 = c * e - b * f, C2 = b * e - c * d;
    const double det = a * C0 + (b * C1 + c * C2);
    if (!(a > 0.0) || !(a * d - b * b > 0.0) || !(det > 0.0)) return false;
    Ji[0] = C0 / det; Ji[1] = C1 / det; Ji[2] = C2 / det;
    Ji[3] = (a * f - c * c) / det; Ji[4] = (b * c - a * e) / det; Ji[5] = (a * d - b * b) / det;
    for (int k = 0; k < 6; ++k) if (!(fabs(Ji[k]) <= 1.79769313486231570815e308)) return false;
    return true;
}

// a rotation matrix (row-major) -> the unit quaternion (w >= 0 branch first; Shepperd's choice of the largest diagonal term)
inline void quaternion_of(const double *R, double *q) {
    const double tr = R[0] + R[4] + R[8];
    double p[4];
    if (tr > 0.0) { const double s = 2.0 * sqrt(1.0 + tr); p[0] = s / 4.0; p[1] = (R[7] - R[5]) / s; p[2] = (R[2] - R[6]) / s; p[3] = (R[3] - R[1]) / s; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]); p[0] = (R[7] - R[5]) / s; p[1] = s / 4.0; p[2] = (R[1] + R[3]) / s; p[3] = (R[2] + R[6]) / s; }
    else if (R[4] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]); p[0] = (R[2] - R[6]) / s; p[1] = (R[1] + R[3]) / s; p[2] = s / 4.0; p[3] = (R[5] + R[7]) / s; }
    else { const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]); p[0] = (R[3] - R[1]) / s; p[1] = (R[2] + R[6]) / s; p[2] = (R[5] + R[7]) / s; p[3] = s / 4.0; }
    normalise(p, q);
}

// a quaternion given from outside: normalised, unless |q|^2 is within 8 ulp of one already -- what this file's normalise leaves, so a
// q read back from a body keeps its bits.  false: a component is not finite or q = 0
inline bool accept_quaternion(const double *p, double *q) {
    for (int k = 0; k < 4; ++k) if (!(fabs(p[k]) <= 1.79769313486231570815e308)) return false;
    const double n2 = p[0] * p[0] + (p[1] * p[1] + (p[2] * p[2] + p[3] * p[3]));
    if (!(n2 > 0.0) || !(n2 <= 1.79769313486231570815e308)) return false;
    if (fabs(n2 - 1.0) <= 8.0 * 2.220446049250313e-16) { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3]; }
    else normalise(p, q);
    return true;
}

} // namespace admm_rigid
