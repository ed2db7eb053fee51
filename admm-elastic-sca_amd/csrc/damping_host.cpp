// damping_host.cpp -- admm_hip_damping_query: the context-free host evaluation of damping.hpp over one group, compiled with
// -ffp-contract=off like the device unit, so that it gives the device's bits (kernels_damping.hpp), the summation order included.
// Needs no GPU and no context.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/admm_hip.h"
#include "damping.hpp"

static_assert(sizeof(admm_hip_group_moments) == sizeof(admm_damping::Moments), "admm_hip_group_moments is damping.hpp's record");

// the two-stage sum of damping.hpp over v[0 .. n)
static double group_sum(const std::vector<double> &v) {
    using namespace admm_damping;
    const size_t n = v.size(), nb = (n + SUM_BLOCK - 1) / SUM_BLOCK;
    std::vector<double> part(nb);
    for (size_t b = 0; b < nb; ++b) {
        double a[SUM_BLOCK];
        for (int i = 0; i < SUM_BLOCK; ++i) { const size_t k = b * SUM_BLOCK + i; a[i] = k < n ? v[k] : 0.0; }
        for (int h = SUM_BLOCK / 2; h >= 1; h >>= 1) for (int i = 0; i < h; ++i) a[i] = a[i] + a[i + h];
        part[b] = a[0];
    }
    double acc[SUM_REDUCE];
    for (int t = 0; t < SUM_REDUCE; ++t) { double s = 0.0; for (size_t i = t; i < nb; i += SUM_REDUCE) s += part[i]; acc[t] = s; }
    for (int h = SUM_REDUCE / 2; h >= 1; h >>= 1) for (int t = 0; t < h; ++t) acc[t] += acc[t + h];
    return acc[0];
}

extern "C" int admm_hip_damping_query(int64_t n, const double *m, const double *x, const double *v, double dt, double drag, double internal,
                                      double *v_out, admm_hip_group_moments *moments) {
    using namespace admm_damping;
    if (n < 1 || !m || !x || !v) return ADMM_ERR_ARG;
    if (!(dt > 0.0) || !(drag >= 0.0) || !(internal >= 0.0) || !std::isfinite(dt) || !std::isfinite(drag) || !std::isfinite(internal)) return ADMM_ERR_ARG;
    Moments R;
    std::memset(&R, 0, sizeof R);
    R.n_nodes = n;
    double vc[3];
    {
        std::vector<double> terms[N_SUMS_1];
        for (int q = 0; q < N_SUMS_1; ++q) terms[q].resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            double t[N_SUMS_1];
            node_terms_1(m[i], x + 3 * (size_t)i, v + 3 * (size_t)i, t);
            for (int q = 0; q < N_SUMS_1; ++q) terms[q][(size_t)i] = t[q];
        }
        double sum[N_SUMS_1];
        for (int q = 0; q < N_SUMS_1; ++q) sum[q] = group_sum(terms[q]);
        finish_1(sum, R, vc);
    }
    {
        std::vector<double> terms[N_SUMS_2];
        for (int q = 0; q < N_SUMS_2; ++q) terms[q].resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            double t[N_SUMS_2];
            node_terms_2(m[i], x + 3 * (size_t)i, v + 3 * (size_t)i, R.com, vc, t);
            for (int q = 0; q < N_SUMS_2; ++q) terms[q][(size_t)i] = t[q];
        }
        double sum[N_SUMS_2];
        for (int q = 0; q < N_SUMS_2; ++q) sum[q] = group_sum(terms[q]);
        finish_2(sum, vc, R);
    }
    if (moments) std::memcpy(moments, &R, sizeof R);
    if (v_out) {
        double beta, s;
        rates(drag, internal, dt, &beta, &s);
        for (int64_t i = 0; i < n; ++i) {
            double w[3] = {v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]};
            if (internal > 0.0) apply_internal(beta, x + 3 * (size_t)i, R.com, vc, R.omega, w);
            if (internal > 0.0 || drag > 0.0) apply_drag(s, w);
            for (int j = 0; j < 3; ++j) v_out[3 * (size_t)i + j] = w[j];
        }
    }
    return ADMM_OK;
}
