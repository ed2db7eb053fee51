// Contact attribution through the class mirror (Settings::contact_attribution, System::contact_owners, entry_resultants): twelve unit-mass
// free nodes, gravity, dt = 0.04, a floor at y = 0 (entry 0) and a sphere of radius 0.5 at (5, 0.2, 0) (entry 1).  Nodes 0 .. 4 start 0.05
// above the floor at 5 m/s downwards, nodes 5 .. 8 start inside the sphere's upper half, nodes 9 .. 11 hang free at y = 3.  Two steps of 10
// iterations from the same state, the second with the switch on; every figure is printed for tests/test_contact_attribution.py, which builds the same scene in Python.
#include <cstdio>
#include <memory>
#include <vector>
#include "admm/System.hpp"
#include "CollisionFloor.hpp"
#include "CollisionSphere.hpp"
#include "CollisionForce.hpp"
using namespace admm;

int main() {
    const int N = 12;
    System system;
    system.settings.verbose = 0;
    system.m_x.resize(3 * N); system.m_v.resize(3 * N); system.m_masses.resize(3 * N);
    system.m_x.fill(0); system.m_v.fill(0); system.m_masses.fill(1);
    for (int i = 0; i < 5; ++i) { system.m_x[3 * i] = 0.25 * i; system.m_x[3 * i + 1] = 0.05; system.m_x[3 * i + 2] = 0.125 * i; }
    for (int i = 5; i < 9; ++i) { system.m_x[3 * i] = 5.0 + 0.125 * (i - 6.5); system.m_x[3 * i + 1] = 0.5 + 0.03125 * (i - 5); system.m_x[3 * i + 2] = 0.0625 * (i - 7); }
    for (int i = 9; i < N; ++i) { system.m_x[3 * i] = 10.0 + i; system.m_x[3 * i + 1] = 3.0; }
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(Vector3d(0, 0, 0))));
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionSphere(Vector3d(5, 0.2, 0), 0.5)));
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    system.settings.timestep_s = 0.04;
    system.settings.admm_iters = 10;
    if (!system.initialize()) return 2;
    for (int i = 0; i < 5; ++i) system.m_v[3 * i + 1] = -5.0;      // (after initialize(), which starts every node at rest)
    const VectorXd x_start = system.m_x, v_start = system.m_v;
    if (!system.step()) return 3;
    if (!system.contact_owners().empty() || !system.entry_resultants(2).empty()) return 4;      // the switch is off: refused
    system.settings.contact_attribution = true;
    system.m_x = x_start; system.m_v = v_start;                    // (the frame again: m_x and m_v travel with every step)
    if (!system.step()) return 5;
    std::vector<admm_hip_contact> c = system.contacts();
    std::vector<admm_hip_contact_owner> o = system.contact_owners();
    if (o.size() != c.size()) return 6;
    for (size_t k = 0; k < o.size(); ++k)
        printf("owner: %d %d normal %.17g %.17g %.17g fn %.17g ft %.17g %.17g %.17g f %.17g %.17g %.17g\n", (int)o[k].node, (int)o[k].entry, o[k].normal[0], o[k].normal[1],
               o[k].normal[2], o[k].f_normal, o[k].f_tangent[0], o[k].f_tangent[1], o[k].f_tangent[2], c[k].f[0], c[k].f[1], c[k].f[2]);
    std::vector<System::ContactResultant> rows = system.entry_resultants(2, 1.0, 0.0, 0.5);
    if (rows.size() != 3) return 7;
    for (size_t q = 0; q < rows.size(); ++q)
        printf("row: %d %ld force %.17g %.17g %.17g torque %.17g %.17g %.17g\n", (int)q, rows[q].count, rows[q].force[0], rows[q].force[1], rows[q].force[2], rows[q].torque[0],
               rows[q].torque[1], rows[q].torque[2]);
    if (!system.entry_resultants(3).empty()) return 8;             // a wrong list length: refused
    return 0;
}
