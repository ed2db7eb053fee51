// attribution.hpp -- which entry of the collision list a contact belongs to, the direction it pushed in, and a reaction's normal and
// tangential parts; shared by the host (attribution_host.cpp: admm_hip_attribution_query) and the device (kernels_collision.hpp form 8,
// kernels_reaction.hpp).  Both sides compile it with -ffp-contract=off and keep the operation order below, so they give the same bits.
// Extension, no reference counterpart.
//
// An entry q of the list MOVED an element's candidate when a coordinate's bits differ between `before`, the point the entry's rule
// started from, and `after`, the point behind the rule and before friction (bits, not values: -0.0 against +0.0 moved, a NaN against
// the same NaN did not; a coordinate that became NaN moved).  An entry that is skipped or whose rule does not fire moved nothing.
//     owner    the index q of the last entry in list order that moved the candidate in that local step; -1: none did
//     normal   of that last mover: d = after - before,  len = sqrt((d0 * d0 + d1 * d1) + d2 * d2),  n_j = d_j / len        three
//              subtractions, five operations and the root, three divides, in that order; owner -1: exactly 0.0.  No scaling: a d whose
//              squares all underflow gives len = 0 and infinite components, a NaN coordinate a NaN normal.
//     split    of a reaction f about a normal n:  fn = (f0 * n0 + f1 * n1) + f2 * n2,  ft_j = f_j - fn * n_j           the product, then
//              the difference
// The normal is the direction of the push: a floor's normal, a sphere's radial, a closed mesh's outward direction at the closest point,
// and for a node mirrored back by side memory or body self-collision the remembered / outer side.
#pragma once
#include "local_math.hpp"

namespace admm_attribution {

ADMM_HD unsigned long long bits(const double v) { unsigned long long b; __builtin_memcpy(&b, &v, sizeof b); return b; }

ADMM_HD bool moved(const double before[3], const double after[3]) {
    return bits(before[0]) != bits(after[0]) || bits(before[1]) != bits(after[1]) || bits(before[2]) != bits(after[2]);
}

// the unit direction of d; call it for a last mover only (owner -1: the normal is 0.0, not this)
ADMM_HD void normal_of(const double d[3], double n[3]) {
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    n[0] = d[0] / len; n[1] = d[1] / len; n[2] = d[2] / len;
}

ADMM_HD void split(const double f[3], const double n[3], double &fn, double ft[3]) {
    fn = (f[0] * n[0] + f[1] * n[1]) + f[2] * n[2];
    ft[0] = f[0] - fn * n[0]; ft[1] = f[1] - fn * n[1]; ft[2] = f[2] - fn * n[2];
}

} // namespace admm_attribution
