// pressure_host.cpp -- admm_hip_pressure_query: the context-free host evaluation of pressure.hpp over one or several chambers, compiled
// with -ffp-contract=off like the device unit, so that it gives the device's bits (kernels_pressure.hpp), the summation order and the
// order of a node's corners included.  Needs no GPU and no context.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/admm_hip.h"
#include "pressure.hpp"
#include "node_csr.hpp"

static_assert(sizeof(admm_hip_chamber_state) == sizeof(admm_pressure::Record), "admm_hip_chamber_state is pressure.hpp's record");
static_assert(ADMM_PRESSURE_CONSTANT == admm_pressure::MODE_CONSTANT && ADMM_PRESSURE_GAS == admm_pressure::MODE_GAS, "pressure.hpp restates the modes");

extern "C" int admm_hip_pressure_query(int64_t nv, const double *x, const double *m, int n_chambers, const int64_t *tri_ptr, const int32_t *tris,
                                       const int32_t *mode, const double *params, double dt, double *dv, admm_hip_chamber_state *records) {
    using namespace admm_pressure;
    if (nv < 1 || nv > 0x7fffffff || !x || !m || n_chambers < 1 || !tri_ptr || !tris || !mode || !params) return ADMM_ERR_ARG;
    if (!(dt > 0.0) || !std::isfinite(dt) || tri_ptr[0] != 0) return ADMM_ERR_ARG;
    for (int c = 0; c < n_chambers; ++c) {
        if (tri_ptr[c + 1] <= tri_ptr[c]) return ADMM_ERR_ARG;
        if (mode[c] != MODE_CONSTANT && mode[c] != MODE_GAS) return ADMM_ERR_ARG;
        if (!std::isfinite(params[2 * c]) || !std::isfinite(params[2 * c + 1])) return ADMM_ERR_ARG;
    }
    const int64_t nt_all = tri_ptr[n_chambers];
    for (int64_t k = 0; k < 3 * nt_all; ++k) if (tris[k] < 0 || tris[k] >= nv) return ADMM_ERR_ARG;
    std::vector<double> nrm(dv ? 3 * (size_t)nt_all : 0);
    std::vector<Record> rec((size_t)n_chambers);
    for (int c = 0; c < n_chambers; ++c) {
        std::memset(&rec[c], 0, sizeof(Record));
        chamber_record(x, tris + 3 * (size_t)tri_ptr[c], tri_ptr[c + 1] - tri_ptr[c], mode[c], params[2 * c], params[2 * c + 1], rec[c], dv ? nrm.data() + 3 * (size_t)tri_ptr[c] : nullptr);
    }
    if (records) std::memcpy(records, rec.data(), sizeof(Record) * (size_t)n_chambers);
    if (!dv) return ADMM_OK;
    // the gather: a node's corners by chamber, then triangle, then corner, inactive chambers left out
    std::vector<admm_lib::NodeCsrEntry> entries;
    entries.reserve(3 * (size_t)nt_all);
    std::vector<int> chamber_of((size_t)nt_all);
    for (int c = 0; c < n_chambers; ++c)
        for (int64_t t = tri_ptr[c]; t < tri_ptr[c + 1]; ++t) {
            chamber_of[(size_t)t] = c;
            for (int j = 0; j < 3; ++j) entries.push_back(admm_lib::NodeCsrEntry{(int)tris[3 * t + j], (long long)t, 1});
        }
    const admm_lib::NodeCsrHost csr = admm_lib::build_node_csr((int)nv, entries);
    for (int64_t i = 0; i < nv; ++i) {
        double f[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
        bool any = false;
        for (int e = csr.ptr[(size_t)i]; e < csr.ptr[(size_t)i + 1]; ++e) {
            const long long t = csr.off[(size_t)e];
            const int c = chamber_of[(size_t)t];
            if (!active(mode[c], params[2 * c], params[2 * c + 1])) continue;
            any = true;
            add_corner(rec[c].pressure, nrm.data() + 3 * (size_t)t, f);
        }
        if (any) increment(dt, f, m[i], d);
        for (int j = 0; j < 3; ++j) dv[3 * (size_t)i + j] = d[j];
    }
    return ADMM_OK;
}
