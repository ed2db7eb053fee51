// Side memory through the class API: a cloth whose nodes carry a thick shell (CollisionSheet::side_reach) over an open obstacle mesh
// (CollisionMesh::side_reach: the cloth's rest triangles, translated), and free particles thrown down at both faster than a frame's
// travel would let the unsigned shell rule catch.  The one CollisionForce's list holds the sheet, then the mesh.
//
//   scene_side_memory <in.bin> <out.bin> <frames> <iters>
// in.bin : int32 nn, ntri, nh, nanch, nc; double x[nn][3], m[nn]; int32 tris[ntri][3], hinges[nh][4], anch[nanch];
//          double sheet half thickness, dt, sheet reach, mesh half thickness, mesh reach, mesh translation y, the particles' start v_y.
//          The cloth is nodes [0, nc); the obstacle mesh's vertices are the cloth's start positions.
// out.bin: frames x (3 nn doubles of m_x, then 3 nn of m_v) after every frame
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "System.hpp"
#include "TriangleForce.hpp"
#include "BendForce.hpp"
#include "AnchorForce.hpp"
#include "CollisionForce.hpp"
#include "ExplicitForce.hpp"

using namespace admm;

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: scene_side_memory in out frames iters\n"); return 1; }
    const int frames = std::atoi(argv[3]), iters = std::atoi(argv[4]);
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 4;
    int32_t hdr[5];
    if (!rd(in, hdr, 5)) return 4;
    const int nn = hdr[0], ntri = hdr[1], nh = hdr[2], nanch = hdr[3], nc = hdr[4];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), tail(7);
    std::vector<int32_t> tris(3 * (size_t)ntri), hinges(4 * (size_t)nh), anch((size_t)nanch);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tris.data(), tris.size()) || !rd(in, hinges.data(), hinges.size()) ||
        !rd(in, anch.data(), anch.size()) || !rd(in, tail.data(), 7)) return 4;
    std::fclose(in);
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = tail[1];
    system.settings.admm_iters = iters;
    Eigen::VectorXd X(3 * nn), M(3 * nn);
    for (int i = 0; i < 3 * nn; ++i) { X[i] = x[i]; M[i] = m[i / 3]; }
    system.add_nodes(X, M);
    for (int t = 0; t < ntri; ++t)
        system.forces.push_back(std::shared_ptr<Force>(new LimitedTriangleStrain(tris[3 * t], tris[3 * t + 1], tris[3 * t + 2], 100.0, 0.95, 1.05)));
    for (int h = 0; h < nh; ++h)
        system.forces.push_back(std::shared_ptr<Force>(new BendForce(hinges[4 * h], hinges[4 * h + 1], hinges[4 * h + 2], hinges[4 * h + 3], 20.0)));
    for (int a = 0; a < nanch; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(anch[a])));
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    const std::vector<int> T(tris.begin(), tris.end());
    std::shared_ptr<CollisionSheet> sheet(new CollisionSheet(0, nc, T, tail[0]));
    sheet->side_reach = tail[2];
    shapes.push_back(sheet);
    std::shared_ptr<CollisionMesh> mesh(new CollisionMesh(Eigen::Vector3d(0, tail[5], 0), std::vector<double>(x.begin(), x.begin() + 3 * (size_t)nc), T, tail[3]));
    mesh->side_reach = tail[4];
    shapes.push_back(mesh);
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;
    for (int i = nc; i < nn; ++i) system.m_v[3 * i + 1] = tail[6];
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) { std::fclose(f); return 3; }
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)nn, f);
        std::fwrite(system.m_v.data(), sizeof(double), 3 * (size_t)nn, f);
    }
    std::fclose(f);
    std::printf("scene_side_memory: %d nodes, %d cloth triangles, %d frames x %d iterations\n", nn, ntri, frames, iters);
    return 0;
}
