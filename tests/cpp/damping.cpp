// Velocity damping per node group through the class mirror (System::add_damping_group, set_damping, group_moments): twelve particles of
// different masses over a far floor, gravity, dt = 0.04, three groups -- internal and drag, drag only, internal only (its rates set
// through set_damping after initialize()).  Two systems step once from the same state: one whose groups have zero rates (it prints the
// state the filter sees, and its moments), one damped.  Every figure is printed with %.17g for tests/test_damping.py.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>
#include "admm/System.hpp"
#include "CollisionFloor.hpp"
#include "CollisionForce.hpp"
using namespace admm;

static const int N = 12;
static const int FIRST[3] = {0, 5, 8}, COUNT[3] = {4, 3, 4};
static const double DRAG[3] = {0.5, 2.0, 0.0}, INTERNAL[3] = {6.0, 0.0, 9.0};

static bool build(System &system, bool damped) {
    system.settings.verbose = 0;
    system.m_x.resize(3 * N); system.m_v.resize(3 * N); system.m_masses.resize(3 * N);
    system.m_v.fill(0);
    for (int i = 0; i < N; ++i) {
        system.m_x[3 * i] = 0.3 * i + 0.1 * std::sin(1.0 + i); system.m_x[3 * i + 1] = 1.0 + 0.2 * std::cos(2.0 * i); system.m_x[3 * i + 2] = 0.25 * ((i * 7) % 5);
        for (int c = 0; c < 3; ++c) system.m_masses[3 * i + c] = 0.5 + 0.125 * i;
    }
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(Vector3d(0, -100, 0))));
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    system.settings.timestep_s = 0.04;
    system.settings.admm_iters = 10;
    for (int g = 0; g < 3; ++g)
        if (system.add_damping_group(FIRST[g], COUNT[g], damped && g < 2 ? DRAG[g] : 0.0, damped && g < 2 ? INTERNAL[g] : 0.0) != g) return false;
    if (!system.initialize()) return false;
    if (system.add_damping_group(4, 1) != -1) return false;                 // after initialize(): refused
    if (damped && !system.set_damping(2, DRAG[2], INTERNAL[2])) return false;
    if (system.set_damping(3, 0.0, 0.0)) return false;                      // no such group
    for (int i = 0; i < N; ++i) {      // (after initialize(), which starts every node at rest)
        system.m_v[3 * i] = 0.4 * std::cos(0.7 * i); system.m_v[3 * i + 1] = -0.3 + 0.1 * i; system.m_v[3 * i + 2] = 0.5 * std::sin(1.3 * i);
    }
    return true;
}

static void print_state(const char *key, System &system) {
    for (int i = 0; i < N; ++i)
        printf("%s: %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", key, i, system.m_masses[3 * i], system.m_x[3 * i], system.m_x[3 * i + 1], system.m_x[3 * i + 2],
               system.m_v[3 * i], system.m_v[3 * i + 1], system.m_v[3 * i + 2]);
}

int main() {
    System plain, damped;
    if (!build(plain, false) || !build(damped, true)) return 2;
    if (!plain.step() || !damped.step()) return 3;
    for (int g = 0; g < 3; ++g) printf("group: %d %d %.17g %.17g\n", FIRST[g], COUNT[g], DRAG[g], INTERNAL[g]);
    print_state("pre", plain);
    print_state("post", damped);
    for (int g = 0; g < 3; ++g) {
        System::GroupMoments r = plain.group_moments(g);
        if (!r.ok) return 4;
        const admm_hip_group_moments &m = r.m;
        printf("moments: %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", m.mass, m.com[0], m.com[1], m.com[2], m.p[0], m.p[1], m.p[2], m.l[0], m.l[1], m.l[2]);
        for (int j = 0; j < 6; ++j) printf(" %.17g", m.inertia[j]);
        printf(" %.17g %.17g %.17g %.17g %.17g %ld %d\n", m.omega[0], m.omega[1], m.omega[2], m.t_total, m.t_rigid, (long)m.n_nodes, (int)m.degenerate);
    }
    if (plain.group_moments(7).ok) return 5;
    return 0;
}
