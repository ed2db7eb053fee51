// anderson_host.cpp -- admm_hip_acceleration_query: the context-free host evaluation of anderson.hpp, compiled with -ffp-contract=off
// like the device unit, so that it gives the device's bits (kernels_anderson.hpp: anderson_decide_kernel).  Needs no GPU and no context.
#include <cstddef>
#include <cstdint>

#include "../../include/admm_hip.h"
#include "anderson.hpp"

extern "C" int admm_hip_acceleration_query(int m_k, const double *gram, const double *rhs, double *theta) {
    if (m_k < 1 || m_k > admm_anderson::MAX_M || !gram || !rhs || !theta) return ADMM_ERR_ARG;
    admm_anderson::solve(m_k, gram, m_k, rhs, theta);      // (not positive definite: theta = 0, as on the device)
    return ADMM_OK;
}
