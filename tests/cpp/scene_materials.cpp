// Consecutive forces of one kind with different constants through the class API: HyperElasticTets that alternate element by
// element between three (mu, lambda, max_iterations) triples, then Springs of per-spring stiffness, then StaticAnchors with
// their own use_weight.  System::initialize merges every run of one kind into ONE batch with per-element parameters.
// usage: scene_materials <in.bin> <out.bin> <frames> <iters>
//   in.bin : int32 n_nodes, n_tets, n_springs, n_anchors; f64 x[3n], m[3n]; int32 tets[4*n_tets]; f64 triples[3][3];
//            int32 springs[2*n_springs]; f64 stiffness[n_springs]; int32 anchors[n_anchors]; f64 use_weight[n_anchors]
//   out.bin: f64 x[3n], v[3n] after every frame, then global_idx / weight of every force as f64
//   stdout : "batches <count>: <kind> x <elements>, ..."
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "admm/System.hpp"
using namespace admm;

struct BatchedSystem : System {      // the batch list is a protected member
    void print_batches() const {
        printf("batches %d:", (int)batch_first.size());
        for (size_t b = 0; b < batch_first.size(); ++b) printf("%s %d x %d", b ? "," : "", batch_kind[b], batch_count[b]);
        printf("\n");
    }
};

int main(int argc, char **argv) {
    if (argc < 5) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int hdr[4];
    if (fread(hdr, sizeof(int), 4, f) != 4) return 1;
    const int n = hdr[0], nt = hdr[1], ns = hdr[2], na = hdr[3];
    std::vector<double> x(3 * n), m(3 * n), ks(ns), uw(na); std::vector<int> tets(4 * nt), springs(2 * ns), anchors(na); double triples[9];
    if (fread(x.data(), 8, 3 * n, f) != (size_t)3 * n || fread(m.data(), 8, 3 * n, f) != (size_t)3 * n) return 1;
    if (fread(tets.data(), 4, 4 * nt, f) != (size_t)4 * nt || fread(triples, 8, 9, f) != 9) return 1;
    if (fread(springs.data(), 4, 2 * ns, f) != (size_t)2 * ns || fread(ks.data(), 8, ns, f) != (size_t)ns) return 1;
    if (fread(anchors.data(), 4, na, f) != (size_t)na || fread(uw.data(), 8, na, f) != (size_t)na) return 1;
    fclose(f);
    const int frames = atoi(argv[3]), iters = atoi(argv[4]);

    BatchedSystem system;
    system.settings.verbose = 0; system.settings.timestep_s = 0.04; system.settings.admm_iters = iters;
    VectorXd xv(3 * n), mv(3 * n);
    for (int i = 0; i < 3 * n; ++i) { xv[i] = x[i]; mv[i] = m[i]; }
    system.add_nodes(xv, mv);
    for (int e = 0; e < nt; ++e) {
        const double *p = triples + 3 * (e % 3);
        system.forces.push_back(std::shared_ptr<Force>(new HyperElasticTet(tets[4 * e], tets[4 * e + 1], tets[4 * e + 2], tets[4 * e + 3], p[0], p[1], (int)p[2], "nh")));
    }
    for (int e = 0; e < ns; ++e) system.forces.push_back(std::shared_ptr<Force>(new Spring(springs[2 * e], springs[2 * e + 1], ks[e])));
    for (int a = 0; a < na; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(anchors[a], uw[a])));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;
    system.print_batches();

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) return 3;
        fwrite(system.m_x.data(), 8, 3 * n, o);
        fwrite(system.m_v.data(), 8, 3 * n, o);
    }
    for (size_t i = 0; i < system.forces.size(); ++i) { double v[2] = {(double)system.forces[i]->global_idx, system.forces[i]->weight}; fwrite(v, 8, 2, o); }
    fclose(o);
    printf("ok %d nodes %d forces\n", n, (int)system.forces.size());
    return 0;
}
