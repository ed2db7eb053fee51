// Pressure chambers through the class mirror (System::add_pressure_chamber, set_pressure, chamber_state): nine particles of different
// masses over a far floor, gravity, dt = 0.04.  Chamber 0 is a closed tetrahedron of particles 0-3 in gas mode (its law set through
// set_pressure after initialize()), chamber 1 two triangles over particles 3-7 at a constant pressure: particle 3 is in both, particle 8
// in none.  Two systems step once: `loaded` with the chambers from v0, `plain` with the same chambers inactive from v0 + dv, dv from
// admm_hip_pressure_query.  Every figure is printed with %.17g for tests/test_pressure.py.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>
#include "admm/System.hpp"
#include "CollisionFloor.hpp"
#include "CollisionForce.hpp"
using namespace admm;

static const int N = 9;
static const int TET[12] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};      // outward normals
static const int FLAP[6] = {3, 4, 5, 5, 6, 7};
static const double AMOUNT = 0.9, AMBIENT = 2.5, P = -3.25, DT = 0.04;

static void v0(double *v) {
    for (int i = 0; i < N; ++i) { v[3 * i] = 0.4 * std::cos(0.7 * i); v[3 * i + 1] = -0.3 + 0.1 * i; v[3 * i + 2] = 0.5 * std::sin(1.3 * i); }
}

static bool build(System &system, bool loaded) {
    system.settings.verbose = 0;
    system.m_x.resize(3 * N); system.m_v.resize(3 * N); system.m_masses.resize(3 * N);
    system.m_v.fill(0);
    const double tet[4][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int i = 0; i < N; ++i) {
        for (int c = 0; c < 3; ++c) {
            system.m_x[3 * i + c] = i < 4 ? 2.0 + 0.8 * tet[i][c] + 0.05 * std::sin(1.0 + 3 * i + c) : 0.3 * i + 0.25 * ((i * 7 + c * 3) % 5) + 0.1 * std::cos(2.0 * i + c);
            system.m_masses[3 * i + c] = 0.5 + 0.125 * i;
        }
    }
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(Vector3d(0, -100, 0))));
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    system.settings.timestep_s = DT;
    system.settings.admm_iters = 10;
    if (system.add_pressure_chamber(std::vector<int>(TET, TET + 12), ADMM_PRESSURE_GAS, 0.0, 0.0) != 0) return false;
    if (system.add_pressure_chamber(std::vector<int>(FLAP, FLAP + 6), ADMM_PRESSURE_CONSTANT, loaded ? P : 0.0) != 1) return false;
    if (!system.initialize()) return false;
    if (system.add_pressure_chamber(std::vector<int>(FLAP, FLAP + 6)) != -1) return false;      // after initialize(): refused
    if (loaded && !system.set_pressure(0, ADMM_PRESSURE_GAS, AMOUNT, AMBIENT)) return false;
    if (system.set_pressure(2, ADMM_PRESSURE_CONSTANT, 1.0)) return false;                        // no such chamber
    v0(&system.m_v[0]);      // (after initialize(), which starts every node at rest)
    return true;
}

int main() {
    System plain, loaded;
    if (!build(plain, false) || !build(loaded, true)) return 2;
    // the twin's increment on the start state
    std::vector<double> x(3 * N), m(N), dv(3 * N);
    for (int i = 0; i < N; ++i) { m[i] = loaded.m_masses[3 * i]; for (int c = 0; c < 3; ++c) x[3 * i + c] = loaded.m_x[3 * i + c]; }
    std::vector<int32_t> tris(TET, TET + 12); tris.insert(tris.end(), FLAP, FLAP + 6);
    const int64_t ptr[3] = {0, 4, 6};
    const int32_t mode[2] = {ADMM_PRESSURE_GAS, ADMM_PRESSURE_CONSTANT};
    const double params[4] = {AMOUNT, AMBIENT, P, 0.0};
    if (admm_hip_pressure_query(N, x.data(), m.data(), 2, ptr, tris.data(), mode, params, DT, dv.data(), nullptr)) return 6;
    printf("law: %d %.17g %.17g\nlaw: %d %.17g %.17g\n", mode[0], AMOUNT, AMBIENT, mode[1], P, 0.0);
    for (int i = 0; i < N; ++i)
        printf("start: %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", i, m[i], x[3 * i], x[3 * i + 1], x[3 * i + 2], loaded.m_v[3 * i], loaded.m_v[3 * i + 1], loaded.m_v[3 * i + 2]);
    for (int c = 0; c < 2; ++c) {      // the records at the start state, before any step
        System::ChamberState r = loaded.chamber_state(c);
        if (!r.ok) return 4;
        const admm_hip_chamber_state &s = r.s;
        printf("record: %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %ld %ld\n", s.volume, s.area, s.area_vector[0], s.area_vector[1], s.area_vector[2], s.pressure,
               s.resultant[0], s.resultant[1], s.resultant[2], (long)s.n_tris, (long)s.collapsed);
    }
    if (loaded.chamber_state(7).ok) return 5;
    for (int k = 0; k < 3 * N; ++k) plain.m_v[k] = plain.m_v[k] + dv[k];
    if (!plain.step() || !loaded.step()) return 3;
    for (int i = 0; i < N; ++i) printf("dv: %d %.17g %.17g %.17g\n", i, dv[3 * i], dv[3 * i + 1], dv[3 * i + 2]);
    for (int i = 0; i < N; ++i) printf("plain: %d %.17g %.17g %.17g %.17g %.17g %.17g\n", i, plain.m_x[3 * i], plain.m_x[3 * i + 1], plain.m_x[3 * i + 2], plain.m_v[3 * i], plain.m_v[3 * i + 1], plain.m_v[3 * i + 2]);
    for (int i = 0; i < N; ++i) printf("loaded: %d %.17g %.17g %.17g %.17g %.17g %.17g\n", i, loaded.m_x[3 * i], loaded.m_x[3 * i + 1], loaded.m_x[3 * i + 2], loaded.m_v[3 * i], loaded.m_v[3 * i + 1], loaded.m_v[3 * i + 2]);
    return 0;
}
