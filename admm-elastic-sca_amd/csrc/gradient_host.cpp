// gradient_host.cpp -- admm_hip_gradient_query, admm_hip_stress_query: the context-free host evaluation of gradient.hpp, compiled with
// -ffp-contract=off like the device unit, so that it gives the device's bits (kernels_gradient.hpp).  Needs no GPU and no context.
#include <cstddef>
#include <cstdint>

#include "../../include/admm_hip.h"
#include "gradient.hpp"

extern "C" int admm_hip_gradient_query(int kind, int64_t n, const double *dx, const double *params, const double *rest, const double *scale, double *g) {
    if (!admm_energy::evaluated(kind) || n < 0) return ADMM_ERR_ARG;
    if (n == 0) return ADMM_OK;
    if (!dx || !params || !rest || !scale || !g) return ADMM_ERR_ARG;
    const int rows = ADMM_KIND_ROWS[kind], np = ADMM_KIND_PARAMS[kind];
    for (int64_t i = 0; i < n; ++i) admm_gradient::element(kind, dx + (size_t)i * rows, params + (size_t)i * np, rest + (size_t)i * 12, scale[i], g + (size_t)i * rows);
    return ADMM_OK;
}

extern "C" int admm_hip_stress_query(int kind, int64_t n, const double *dx, const double *params, const double *volume, double *stress7) {
    if (!admm_gradient::is_tet(kind) || n < 0) return ADMM_ERR_ARG;
    if (n == 0) return ADMM_OK;
    if (!dx || !params || !volume || !stress7) return ADMM_ERR_ARG;
    const int np = ADMM_KIND_PARAMS[kind];
    const double rest[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // (no tet kind reads it)
    for (int64_t i = 0; i < n; ++i) {
        const double *d = dx + (size_t)i * 9, *par = params + (size_t)i * np;
        double g[9];
        admm_gradient::element(kind, d, par, rest, admm_gradient::tet_scale(kind, par, volume[i]), g);
        admm_gradient::tet_stress(admm_energy::mat_from_rows(d), g, volume[i], stress7 + (size_t)i * 7);
    }
    return ADMM_OK;
}
