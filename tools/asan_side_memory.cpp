// The host routines of side memory (csrc/mesh.cpp: the boundary table of admm_hip_mesh_create_open, admm_hip_mesh_side_latch,
// admm_hip_mesh_query_sided, admm_hip_mesh_feature_normal) in a stand-alone program for AddressSanitizer + UBSan: tools/asan_side_memory.sh
// compiles it with mesh.cpp under -fsanitize=address,undefined and runs it.  Meshes: an n x n grid, a bent copy of it (set_vertices),
// a single triangle, a closed tetrahedron; points in and far around the boxes, with and without a translation and a frame.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/admm_hip.h"

static double urand() { return std::rand() / (double)RAND_MAX; }

static int run(admm_hip_mesh *m, double r, double R, int nt, long &crossed_total) {
    std::vector<int32_t> bits(nt), orig(nt);
    if (admm_hip_mesh_boundary_table(m, bits.data(), orig.data())) return 1;
    for (int i = 0; i < nt; ++i) if (orig[i] < 0 || orig[i] >= nt || (bits[i] & ~0x7e)) return 2;
    const int n = 4000;
    std::vector<double> P(3 * n), proj(3 * n), sd(n), nr(3 * n);
    std::vector<int32_t> prev(n), side(n), tri(n), cr(n), slot(n), reg(n);
    for (int i = 0; i < n; ++i) {
        const double s = i % 7 == 0 ? 20.0 : 1.5;
        for (int j = 0; j < 3; ++j) P[3 * i + j] = s * (urand() - 0.5);
        if (i % 3) P[3 * i + 1] *= 0.2;
        prev[i] = std::rand() % 3 - 1;
    }
    const double c = std::cos(0.7), s = std::sin(0.7);
    const double frame[12] = {c, -s, 0, s, c, 0, 0, 0, 1, 0.1, -0.2, 0.3};
    const double t0[3] = {0, 0, 0}, t1[3] = {0.25, -0.125, 0.5};
    for (int pass = 0; pass < 4; ++pass) {
        const double *t = pass & 1 ? t1 : t0;
        const double *f = pass & 2 ? frame : nullptr;
        if (admm_hip_mesh_side_latch(m, n, P.data(), pass ? prev.data() : nullptr, R, t, f, side.data())) return 3;
        if (admm_hip_mesh_query_sided(m, n, P.data(), side.data(), R, t, f, proj.data(), sd.data(), tri.data(), cr.data())) return 4;
        if (admm_hip_mesh_query_sided(m, n, P.data(), prev.data(), R, t, f, proj.data(), nullptr, nullptr, cr.data())) return 5;
        for (int i = 0; i < n; ++i) { crossed_total += cr[i]; if (side[i] < -1 || side[i] > 1 || !std::isfinite(proj[3 * i])) return 6; }
        if (admm_hip_mesh_query_sided(m, n, P.data(), nullptr, R, t, f, nullptr, sd.data(), tri.data(), nullptr)) return 7;
    }
    if (admm_hip_mesh_closest(m, n, P.data(), R * R, nullptr, nullptr, slot.data(), reg.data(), nullptr)) return 8;
    for (int i = 0; i < n; ++i) if (slot[i] < 0) { slot[i] = 0; reg[i] = 0; }
    if (admm_hip_mesh_feature_normal(m, n, slot.data(), reg.data(), nr.data())) return 9;
    slot[0] = nt;
    if (admm_hip_mesh_feature_normal(m, n, slot.data(), reg.data(), nr.data()) != ADMM_ERR_ARG) return 10;
    prev[5] = 2;
    if (admm_hip_mesh_side_latch(m, n, P.data(), prev.data(), R, t0, nullptr, side.data()) != ADMM_ERR_ARG) return 11;
    if (admm_hip_mesh_query_sided(m, n, P.data(), prev.data(), R, t0, nullptr, proj.data(), nullptr, nullptr, nullptr) != ADMM_ERR_ARG) return 12;
    if (admm_hip_mesh_side_latch(m, n, P.data(), nullptr, 0.5 * r, t0, nullptr, side.data()) != ADMM_ERR_ARG) return 13;
    return 0;
}

int main() {
    std::srand(7);
    char err[512];
    long crossed = 0;
    for (int ng : {1, 4, 9}) {
        std::vector<double> V; std::vector<int32_t> F;
        for (int j = 0; j <= ng; ++j) for (int i = 0; i <= ng; ++i) { V.push_back(i / (double)ng - 0.5); V.push_back(0.0); V.push_back(j / (double)ng - 0.5); }
        for (int j = 0; j < ng; ++j) for (int i = 0; i < ng; ++i) {
            const int a = j * (ng + 1) + i, b = a + 1, c = a + ng + 1, d = c + 1;
            F.insert(F.end(), {a, c, b, b, c, d});
        }
        admm_hip_mesh *m = nullptr;
        const double r = 0.0625, R = 0.25;
        if (admm_hip_mesh_create_open(&m, (int)V.size() / 3, V.data(), (int)F.size() / 3, F.data(), r, err, sizeof err)) { std::fprintf(stderr, "%s\n", err); return 20; }
        int rc = run(m, r, R, (int)F.size() / 3, crossed);
        if (rc) { std::fprintf(stderr, "grid %d: step %d\n", ng, rc); return rc; }
        for (size_t k = 0; k < V.size() / 3; ++k) V[3 * k + 1] = 0.3 * V[3 * k] * V[3 * k] - 0.2 * V[3 * k + 2] * V[3 * k];      // bent: the table stays, the normals change
        if (admm_hip_mesh_set_vertices(m, (int)V.size() / 3, V.data(), err, sizeof err)) { std::fprintf(stderr, "%s\n", err); return 21; }
        rc = run(m, r, R, (int)F.size() / 3, crossed);
        if (rc) { std::fprintf(stderr, "bent grid %d: step %d\n", ng, rc); return rc; }
        admm_hip_mesh_destroy(m);
    }
    {   // a closed mesh: an all-zero table, and the sided routines refuse it
        const double V[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
        const int32_t F[12] = {0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2};
        admm_hip_mesh *m = nullptr;
        if (admm_hip_mesh_create(&m, 4, V, 4, F, err, sizeof err)) { std::fprintf(stderr, "%s\n", err); return 22; }
        int32_t bits[4], side[1]; const double P[3] = {0.1, 0.1, 0.1}, t[3] = {0, 0, 0};
        if (admm_hip_mesh_boundary_table(m, bits, nullptr) || bits[0] || bits[1] || bits[2] || bits[3]) return 23;
        if (admm_hip_mesh_side_latch(m, 1, P, nullptr, 0.5, t, nullptr, side) != ADMM_ERR_ARG) return 24;
        admm_hip_mesh_destroy(m);
    }
    std::printf("asan_side_memory: ok (%ld crossed projections)\n", crossed);
    return crossed > 1000 ? 0 : 30;
}
