"""What friction costs the collision launch: the 32 x 32 x 163 bar (1M Neo-Hookean tets, 178 596 nodes) resting on a floor, one collision
element per node, a few frames with every coefficient 0 (project_collision_kernel) and the same frames on a twin with mu = 0.5
(project_collision_friction_kernel).  One launch per batch and no graphs, so that a kernel trace shows the collision launch under its own name:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -- python tools/probe_friction.py

and compare the two kernels' average times in the statistics.  The friction form gathers 24 more bytes per node (the frame-start x)."""
import os
import sys

os.environ["ADMM_HIP_LOCAL_MULTI"] = "0"
os.environ["ADMM_HIP_GRAPH"] = "0"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def scene(pkg, mu, nx=32, ny=32, nz=163):
    mg = pkg.meshgen
    x, tets = mg.bar(nx, ny, nz)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    s = pkg.System(device_id=0)
    s.set_timestep(0.04)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(pkg.KIND["TET_NH"], tets, [1e5, 1e5, 5])
    s.add_forces(pkg.KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity((0.0, -9.8, 0.0))
    s.set_collision_shapes([pkg.SHAPE["FLOOR"]], [[0.0, 0.0, 0.0, 0.0]])
    s.set_collision_friction([mu])
    s.initialize()
    return s, len(x)


def main():
    pkg = load_package()
    frames, iters = 5, 20
    for mu in (0.0, 0.5):
        s, n = scene(pkg, mu)
        for _ in range(frames):
            s.step(iters)
        s.sync()
        y = s.m_x.reshape(-1, 3)[:, 1]
        print("mu %.1f: %d nodes, %d frames x %d iterations, %d nodes within 1 mm of the floor" % (mu, n, frames, iters, int((y < 1e-3).sum())))
        del s


if __name__ == "__main__":
    main()
