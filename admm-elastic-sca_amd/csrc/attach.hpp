// attach.hpp -- rigid attachments: a whole ANCHOR batch fastened to a rigid body of the collision list (rigid.hpp).  The batch's targets
// ride with the body's pose, and the reaction of its active elements loads the body next to its contacts.  Shared by the host
// (attach_host.cpp: admm_hip_attachment_query; abi_attach.inc: registration) and the device (kernels_attach.hpp).  Both sides compile it
// with -ffp-contract=off and keep the operation order below, so they give the same bits.  Only + - * /, no libm call.  Extension, no
// reference counterpart.
//
// With c[3] the body's centre of mass and R[9] its rotation (row-major), as admm_rigid::Record holds them.  Every product is rounded,
// sums are associated as written, no fused multiply-adds:
//   local offset (host only, at attachment), from an element's target t:
//              e_j = t_j - c_j;   r_j = R_0j e_0 + (R_1j e_1 + R_2j e_2)                      r = R^T (t - c)
//   target (device, at the start of every frame; host query), from the record as the frame before left it:
//              t_j = c_j + (R_j0 r_0 + (R_j1 r_1 + R_j2 r_2))                                  t = c + R r
//     A target recomputed from a derived offset may differ from the one the offset came from in the last bits.
//   load, per attached element, after the frame's epilogue:
//              active != 0:  f = admm_reaction::force(w2, u, z, x);  the six terms admm_reaction::resultant_terms(f, z, c)
//              active == 0:  six +0.0
//     u, z: what the frame's last local step stored; x: the final position; c: the body's centre BEFORE this frame's integration, the
//     pivot of its contact row.
//   sum, per body and per component of the six terms, over the body's attached elements in ascending (batch index, device element
//     index) -- the order of admm_hip_read_local -- in reaction.hpp's two-stage order: blocks of 64 consecutive elements, the last one
//     padded with +0.0, folded a[i] = a[i] + a[i + h], h = 32 .. 1; then the 256-lane second stage over the blocks' partials.
//   combined with the contacts, only for a body that carries at least one attached batch:
//              Fe_j = Fc_j + Fa_j;   Te_j = Tc_j + Ta_j          one rounded add each; admm_rigid::step then runs unchanged
//     A body without a batch does not take the add (-0.0 + 0.0 would flip a sign bit of F): it keeps the bits it had.
#pragma once
#include "reaction.hpp"

namespace admm_attach {

// r = R^T (t - c)
inline void local_offset(const double *c, const double *R, const double *t, double *r) {
    const double e0 = t[0] - c[0], e1 = t[1] - c[1], e2 = t[2] - c[2];
    r[0] = R[0] * e0 + (R[3] * e1 + R[6] * e2);
    r[1] = R[1] * e0 + (R[4] * e1 + R[7] * e2);
    r[2] = R[2] * e0 + (R[5] * e1 + R[8] * e2);
}

// t = c + R r
ADMM_HD void target(const double *c, const double *R, const double *r, double *t) {
    t[0] = c[0] + (R[0] * r[0] + (R[1] * r[1] + R[2] * r[2]));
    t[1] = c[1] + (R[3] * r[0] + (R[4] * r[1] + R[5] * r[2]));
    t[2] = c[2] + (R[6] * r[0] + (R[7] * r[1] + R[8] * r[2]));
}

// an element's six terms of its body's attachment row about `pivot`
ADMM_HD void load_terms(const int active, const double w2, const double *u, const double *z, const double *x, const double *pivot, double *t) {
    if (active != 0) {
        double f[3];
        admm_reaction::force(w2, u, z, x, f);
        admm_reaction::resultant_terms(f, z, pivot, t);
    } else {
        t[0] = 0.0; t[1] = 0.0; t[2] = 0.0; t[3] = 0.0; t[4] = 0.0; t[5] = 0.0;
    }
}

// the contacts' and the attachments' component of a body's row
ADMM_HD double combine(const double contact, const double attached) { return contact + attached; }

} // namespace admm_attach
