// attach_host.cpp -- admm_hip_attachment_query: the context-free host evaluation of attach.hpp, compiled with -ffp-contract=off like the
// device unit, so that it gives the device's bits (kernels_attach.hpp), the row's summation order included.  Needs no GPU and no context.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/admm_hip.h"
#include "attach.hpp"

// the two-stage sum of reaction.hpp over v[0 .. n)
static double attach_row_sum(const std::vector<double> &v) {
    using namespace admm_reaction;
    const size_t n = v.size(), nb = (n + RESULTANT_BLOCK - 1) / RESULTANT_BLOCK;
    std::vector<double> part(nb);
    for (size_t b = 0; b < nb; ++b) {
        double a[RESULTANT_BLOCK];
        for (int i = 0; i < RESULTANT_BLOCK; ++i) { const size_t k = b * RESULTANT_BLOCK + i; a[i] = k < n ? v[k] : 0.0; }
        for (int h = RESULTANT_BLOCK / 2; h >= 1; h >>= 1) for (int i = 0; i < h; ++i) a[i] = a[i] + a[i + h];
        part[b] = a[0];
    }
    double acc[RESULTANT_REDUCE];
    for (int t = 0; t < RESULTANT_REDUCE; ++t) { double s = 0.0; for (size_t i = t; i < nb; i += RESULTANT_REDUCE) s += part[i]; acc[t] = s; }
    for (int h = RESULTANT_REDUCE / 2; h >= 1; h >>= 1) for (int t = 0; t < h; ++t) acc[t] += acc[t + h];
    return acc[0];
}

extern "C" int admm_hip_attachment_query(int64_t n, const double c[3], const double R[9], const double *local, double *targets, const double *f, const double *point,
                                         const int32_t *active, const double pivot[3], double *row6, int64_t *n_active) {
    if (n < 0) return ADMM_ERR_ARG;
    if (targets) {      // the target half
        if (!c || !R || (n > 0 && !local)) return ADMM_ERR_ARG;
        for (int64_t i = 0; i < n; ++i) admm_attach::target(c, R, local + 3 * (size_t)i, targets + 3 * (size_t)i);
    }
    if (row6 || n_active) {      // the sum half
        if (n > 0 && (!f || !point)) return ADMM_ERR_ARG;
        const double origin[3] = {0.0, 0.0, 0.0};
        const double *pv = pivot ? pivot : origin;
        std::vector<double> terms[6];
        for (int r = 0; r < 6; ++r) terms[r].resize((size_t)n);
        int64_t na = 0;
        for (int64_t i = 0; i < n; ++i) {
            double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (!active || active[i] != 0) { admm_reaction::resultant_terms(f + 3 * (size_t)i, point + 3 * (size_t)i, pv, t); ++na; }
            for (int r = 0; r < 6; ++r) terms[r][(size_t)i] = t[r];
        }
        if (row6) for (int r = 0; r < 6; ++r) row6[r] = attach_row_sum(terms[r]);
        if (n_active) *n_active = na;
    }
    return ADMM_OK;
}
