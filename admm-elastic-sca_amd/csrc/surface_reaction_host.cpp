// surface_reaction_host.cpp -- admm_hip_surface_reaction_query: the context-free host evaluation of surface_reaction.hpp's shares and
// ordered sums, compiled with -ffp-contract=off like the device unit, so that it gives the device's bits
// (kernels_surface_reaction.hpp): a node's contributions in ascending (contact, corner).  Needs no GPU and no context.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/admm_hip.h"
#include "surface_reaction.hpp"

static_assert(sizeof(admm_hip_surface_contact) == sizeof(admm_surface_reaction::Record), "admm_hip_surface_contact is surface_reaction.hpp's record");
static_assert((int)ADMM_SURFACE_REACTING == (int)admm_surface_reaction::REACTING && (int)ADMM_SURFACE_UNOWNED == (int)admm_surface_reaction::UNOWNED &&
              (int)ADMM_SURFACE_OTHER == (int)admm_surface_reaction::OTHER && (int)ADMM_SURFACE_SELF == (int)admm_surface_reaction::SELF, "surface_reaction.hpp restates the statuses");

extern "C" int admm_hip_surface_reaction_query(int64_t n_nodes, const double *m3, int64_t K, const double *f, const int32_t *corner, const double *weight,
                                               const double *share, double dt, double *dv) {
    using namespace admm_surface_reaction;
    if (n_nodes < 1 || n_nodes > 0x7fffffff || !m3 || K < 0 || !dv) return ADMM_ERR_ARG;
    if (K && (!f || !corner || !weight || !share)) return ADMM_ERR_ARG;
    if (!(dt > 0.0) || !std::isfinite(dt)) return ADMM_ERR_ARG;
    for (int64_t k = 0; k < K; ++k) {
        if (!(share[k] >= 0.0 && share[k] <= 1.0)) return ADMM_ERR_ARG;
        if (share[k] > 0.0) for (int c = 0; c < 3; ++c) if (corner[3 * k + c] < 0 || corner[3 * k + c] >= n_nodes) return ADMM_ERR_ARG;
    }
    // the inverted index: per destination node its (contact, corner) pairs, ascending -- a counting sort by node keeps that order
    std::vector<int64_t> ptr((size_t)n_nodes + 1, 0);
    for (int64_t k = 0; k < K; ++k) if (share[k] > 0.0) for (int c = 0; c < 3; ++c) ++ptr[(size_t)corner[3 * k + c] + 1];
    for (int64_t i = 0; i < n_nodes; ++i) ptr[(size_t)i + 1] += ptr[(size_t)i];
    std::vector<int64_t> list((size_t)ptr[(size_t)n_nodes]), fill(ptr.begin(), ptr.end() - 1);
    for (int64_t k = 0; k < K; ++k) if (share[k] > 0.0) for (int c = 0; c < 3; ++c) list[(size_t)fill[(size_t)corner[3 * k + c]]++] = 3 * k + c;
    for (int64_t i = 0; i < n_nodes; ++i) {
        double d[3] = {0.0, 0.0, 0.0};
        if (ptr[(size_t)i + 1] > ptr[(size_t)i]) {
            double a[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
            for (int64_t e = ptr[(size_t)i]; e < ptr[(size_t)i + 1]; ++e) {
                const int64_t k = list[(size_t)e] / 3;
                double p[3], q[3];
                impulse(dt, f + 3 * k, p);
                contribution(share[k], weight[list[(size_t)e]], p, q);
                accumulate(q, a);
            }
            apply(a, m3 + 3 * (size_t)i, d, v);
        }
        for (int j = 0; j < 3; ++j) dv[3 * (size_t)i + j] = d[j];
    }
    return ADMM_OK;
}
