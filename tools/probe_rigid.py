"""What a rigid body costs a frame: a bar of nx x ny x nz cells (default 8 x 8 x 40: 15 360 Neo-Hookean tets, 3 321 nodes) anchored at one
end, one collision element per node, contact attribution on, a sphere resting 1 mm above its top -- the same frames with the sphere left
kinematic and with it registered as a rigid body under gravity (admm_hip_add_rigid_body: per frame the pose launch, the reaction and
attribution reports' launches, entry_count / row_scan / entry_place, rigid_partial / reduce / integrate).  Prints the wall time per frame of both,
synchronised once at the end; the first frames (graph capture) are left out.

    timeout -k 10 300 python tools/probe_rigid.py [nx ny nz]

The numbers are a report, nothing is asserted."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def scene(pkg, dynamic, nx, ny, nz):
    mg = pkg.meshgen
    x, tets = mg.bar(nx, ny, nz)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    s = pkg.System(device_id=0)
    s.set_timestep(0.02)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(pkg.KIND["TET_NH"], tets, [1e5, 1e5, 5])
    s.add_forces(pkg.KIND["ANCHOR"], mg.bar_anchor_nodes(nx, ny), [1000.0, 1.0])
    s.add_forces(pkg.KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity((0.0, -9.8, 0.0))
    r = 0.1
    c = [0.05 * nx / 2, 0.05 * ny + r + 0.001, 0.05 * nz / 2]
    s.set_collision_shapes([pkg.SHAPE["SPHERE"]], [c + [r]])
    s.enable_contact_attribution(True)
    if dynamic:
        M = 0.25 * float(m.sum())
        s.add_rigid_body(0, M, [0.4 * M * r * r * d for d in (1, 0, 0, 1, 0, 1)], c, (0.0, -9.8, 0.0))
    s.initialize()
    return s, len(x), len(tets)


def main():
    pkg = load_package()
    dims = [int(a) for a in sys.argv[1:4]] if len(sys.argv) >= 4 else [8, 8, 40]
    warm, frames, iters = 5, 40, 10
    for dynamic in (False, True):
        s, n, nt = scene(pkg, dynamic, *dims)
        for _ in range(warm):
            s.step(iters)
        s.sync()
        t0 = time.perf_counter()
        for _ in range(frames):
            s.step(iters)
        s.sync()
        ms = 1e3 * (time.perf_counter() - t0) / frames
        tail = ""
        if dynamic:
            r = s.rigid_state()[0]
            tail = "; the sphere's centre y %.4f, %d contacts, F_y %.3g N" % (r.c[1], r.count, r.F[1])
        print("%s: %d nodes, %d tets, %d frames x %d iterations: %.3f ms per frame%s" % ("dynamic  " if dynamic else "kinematic", n, nt, frames, iters, ms, tail))
        del s


if __name__ == "__main__":
    main()
