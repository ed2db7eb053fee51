// reaction_host.cpp -- admm_hip_reaction_query: the context-free host evaluation of reaction.hpp, compiled with -ffp-contract=off like
// the device unit, so that it gives the device's bits (kernels_reaction.hpp), the resultant's summation order included.  Needs no GPU
// and no context.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/admm_hip.h"
#include "reaction.hpp"

// the two-stage sum of reaction.hpp over v[0 .. n)
static double resultant_sum(const std::vector<double> &v) {
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

extern "C" int admm_hip_reaction_query(int64_t n, const double *w2, const double *u, const double *z, const double *x, double depth_min, const double *pivot,
                                       double *f, double *depth, int32_t *flag, double *resultant6) {
    if (n < 0 || !(depth_min >= 0.0)) return ADMM_ERR_ARG;
    if (n > 0 && (!w2 || !u || !z || !x)) return ADMM_ERR_ARG;
    const double origin[3] = {0.0, 0.0, 0.0};
    const double *pv = pivot ? pivot : origin;
    std::vector<double> terms[6];
    for (int64_t i = 0; i < n; ++i) {
        double fi[3];
        admm_reaction::force(w2[i], u + 3 * (size_t)i, z + 3 * (size_t)i, x + 3 * (size_t)i, fi);
        const double d = admm_reaction::depth(u + 3 * (size_t)i);
        const bool c = admm_reaction::in_contact(d, depth_min);
        if (f) for (int j = 0; j < 3; ++j) f[3 * (size_t)i + j] = fi[j];
        if (depth) depth[i] = d;
        if (flag) flag[i] = c ? 1 : 0;
        if (resultant6 && c) {
            double t[6];
            admm_reaction::resultant_terms(fi, z + 3 * (size_t)i, pv, t);
            for (int r = 0; r < 6; ++r) terms[r].push_back(t[r]);
        }
    }
    if (resultant6) for (int r = 0; r < 6; ++r) resultant6[r] = resultant_sum(terms[r]);
    return ADMM_OK;
}
