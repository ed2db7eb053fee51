// rigid_host.cpp -- admm_hip_rigid_query: the context-free host evaluation of rigid.hpp's frame for one body, compiled with
// -ffp-contract=off like the device unit, so that it gives the device's bits (kernels_rigid.hpp: rigid_integrate_kernel).  Needs no GPU
// and no context.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/admm_hip.h"
#include "rigid.hpp"

static_assert(sizeof(admm_hip_rigid_state) == sizeof(admm_rigid::Record), "admm_hip_rigid_state is rigid.hpp's record");
static_assert(offsetof(admm_hip_rigid_state, count) == offsetof(admm_rigid::Record, count) && offsetof(admm_hip_rigid_state, par) == offsetof(admm_rigid::Record, par),
              "admm_hip_rigid_state is rigid.hpp's record");

extern "C" int admm_hip_rigid_query(int type, double mass, const double inertia[6], const double accel[3], const double c0[3], const double par0[4],
                                    const admm_hip_rigid_state *in, const double Fe[3], const double Te[3], int64_t count, double dt, admm_hip_rigid_state *out) {
    using namespace admm_rigid;
    if (!inertia || !in || !Fe || !Te || !out) return ADMM_ERR_ARG;
    if (!(mass > 0.0) || !std::isfinite(mass) || !(dt > 0.0) || !std::isfinite(dt)) return ADMM_ERR_ARG;
    Const K{};
    K.mass = mass; K.entry = in->entry; K.type = type;
    if (!invert_inertia(inertia, K.Jinv)) return ADMM_ERR_ARG;
    for (int j = 0; j < 3; ++j) { K.accel[j] = accel ? accel[j] : 0.0; K.c0[j] = c0 ? c0[j] : in->c[j]; }
    for (int j = 0; j < 4; ++j) K.par0[j] = par0 ? par0[j] : in->par[j];
    Record S, O;
    static_assert(sizeof S == sizeof *in, "one record");
    std::memcpy(&S, in, sizeof S);
    step(K, S, Fe, Te, count, dt, O);
    std::memcpy(out, &O, sizeof O);
    return ADMM_OK;
}
