// attribution_host.cpp -- admm_hip_attribution_query: the context-free host evaluation of attribution.hpp, compiled with
// -ffp-contract=off like the device unit, so that it gives the device's bits (kernels_collision.hpp form 8, kernels_reaction.hpp).
// Needs no GPU and no context.
#include <cstddef>
#include <cstdint>

#include "../../include/admm_hip.h"
#include "attribution.hpp"

extern "C" int admm_hip_attribution_query(int64_t n, const double *before, const double *after, const double *f, const double *normal_in, int32_t *moved, double *normal,
                                          double *fn, double *ft) {
    if (n < 0) return ADMM_ERR_ARG;
    const bool pts = before && after;
    if (n > 0 && !pts && (before || after || !normal_in)) return ADMM_ERR_ARG;      // both points, or neither and the normals given
    if (n > 0 && !f && (fn || ft)) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        bool mv = false;
        double nr[3] = {0.0, 0.0, 0.0};
        if (pts) {
            const double *b = before + 3 * (size_t)i, *a = after + 3 * (size_t)i;
            mv = admm_attribution::moved(b, a);
            if (mv) { const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; admm_attribution::normal_of(d, nr); }
        }
        if (moved) moved[i] = mv ? 1 : 0;
        if (normal) for (int j = 0; j < 3; ++j) normal[3 * (size_t)i + j] = nr[j];
        if (f && (fn || ft)) {
            double s, t[3];
            admm_attribution::split(f + 3 * (size_t)i, normal_in ? normal_in + 3 * (size_t)i : nr, s, t);
            if (fn) fn[i] = s;
            if (ft) for (int j = 0; j < 3; ++j) ft[3 * (size_t)i + j] = t[j];
        }
    }
    return ADMM_OK;
}
