// Contact and anchor reactions through the class mirror (System::node_reactions, contacts, contact_resultant): three unit-mass nodes,
// gravity, dt = 0.04.  Node 0 starts 0.05 above a floor at y = 0 at 5 m/s downwards and hits it within the frame, node 1 hangs free
// at y = 1, node 2 is held by a StaticAnchor.  One step of 10 iterations; every figure is printed for tests/test_reactions.py.
#include <cstdio>
#include <memory>
#include <vector>
#include "admm/System.hpp"
#include "CollisionFloor.hpp"
#include "CollisionForce.hpp"
using namespace admm;

int main() {
    System system;
    system.settings.verbose = 0;
    system.m_x.resize(9); system.m_v.resize(9); system.m_masses.resize(9);
    system.m_x.fill(0); system.m_v.fill(0); system.m_masses.fill(1);
    system.m_x[1] = 0.05;
    system.m_x[3] = 1.0; system.m_x[4] = 1.0;
    system.m_x[6] = 2.0; system.m_x[7] = 1.0;
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(Vector3d(0, 0, 0))));
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(2)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    system.settings.timestep_s = 0.04;
    if (!system.initialize()) return 2;
    if (system.node_reactions().ok || !system.contacts().empty() || system.contact_resultant().count != -1) return 4;      // no step yet: refused
    system.settings.admm_iters = 10;
    system.m_v[1] = -5.0;      // (after initialize(), which starts every node at rest; m_x and m_v travel with every step)
    if (!system.step()) return 3;
    System::NodeReactions r = system.node_reactions();
    if (!r.ok) return 5;
    printf("info: %ld %ld %ld %ld\n", r.batches_collision, r.batches_anchor, r.batches_skipped, r.n_contacts);
    for (int i = 0; i < 3; ++i)
        printf("node: %d x %.17g %.17g %.17g contact %.17g %.17g %.17g anchor %.17g %.17g %.17g\n", i, system.m_x[3 * i], system.m_x[3 * i + 1], system.m_x[3 * i + 2],
               r.contact[3 * i], r.contact[3 * i + 1], r.contact[3 * i + 2], r.anchor[3 * i], r.anchor[3 * i + 1], r.anchor[3 * i + 2]);
    std::vector<admm_hip_contact> c = system.contacts();
    for (size_t k = 0; k < c.size(); ++k)
        printf("contact: %d f %.17g %.17g %.17g point %.17g %.17g %.17g depth %.17g\n", (int)c[k].node, c[k].f[0], c[k].f[1], c[k].f[2], c[k].point[0], c[k].point[1], c[k].point[2], c[k].depth);
    System::ContactResultant t = system.contact_resultant(1.0, 0.0, 0.0);
    printf("resultant: %ld force %.17g %.17g %.17g torque %.17g %.17g %.17g\n", t.count, t.force[0], t.force[1], t.force[2], t.torque[0], t.torque[1], t.torque[2]);
    return 0;
}
