// energy_host.cpp -- admm_hip_energy_query: the context-free host evaluation of energy.hpp, compiled with -ffp-contract=off like the
// device unit, so that it gives the device's bits (kernels_energy.hpp).  Needs no GPU and no context.
#include <cstddef>
#include <cstdint>

#include "../../include/admm_hip.h"
#include "energy.hpp"

extern "C" int admm_hip_energy_query(int kind, int64_t n, const double *dx, const double *params, const double *rest, const double *scale, double *energy) {
    if (!admm_energy::evaluated(kind) || n < 0) return ADMM_ERR_ARG;
    if (n == 0) return ADMM_OK;
    if (!dx || !params || !rest || !scale || !energy) return ADMM_ERR_ARG;
    const int rows = ADMM_KIND_ROWS[kind], np = ADMM_KIND_PARAMS[kind];
    for (int64_t i = 0; i < n; ++i) energy[i] = admm_energy::element(kind, dx + (size_t)i * rows, params + (size_t)i * np, rest + (size_t)i * 12, scale[i]);
    return ADMM_OK;
}
