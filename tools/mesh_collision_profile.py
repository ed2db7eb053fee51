#!/usr/bin/env python3
"""The mesh-collision launch on the headline bar (32x32x163 cubes, 178 596 nodes): a collision batch over all nodes whose shape list is
ONE level-6 icosphere (81 920 triangles) of radius 0.6 centred on the bar's axis halfway along it (`mesh`), or an analytic sphere of the
same radius and centre (`sphere`), or the icosphere turned about its centre with a friction coefficient (`framed`: every element on
project_collision_framed_kernel<true>, the lowest instantiation of the body that forms 3 to 7 share).
Run under  rocprofv3 --kernel-trace --stats -- python tools/mesh_collision_profile.py mesh|sphere|framed
usage: mesh_collision_profile.py mesh|sphere|framed [frames=3] [iters=10] [nx ny nz]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package
from test_collision_frames import _frame, _rot
from test_collision_mesh import icosphere

pkg = load_package()
mode = sys.argv[1]
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 3
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
nx, ny, nz = (int(v) for v in sys.argv[4:7]) if len(sys.argv) > 6 else (32, 32, 163)
h, R = 0.05, 0.6
s = pkg.make_bar_system(nx, ny, nz, device_id=0, h=h)
n = (nx + 1) * (ny + 1) * (nz + 1)
s.add_forces(pkg.KIND["COLLISION"], np.arange(n, dtype=np.int32), [32.0])
c = np.array([nx * h / 2, ny * h / 2, nz * h / 2])
if mode in ("mesh", "framed"):
    V, F = icosphere(6, R)
    mid = s.add_collision_mesh(V, F)
    s.set_collision_shapes([pkg.SHAPE["MESH"]], [[*c, mid]])
    if mode == "framed":
        s.set_collision_friction([0.3])
        s.set_collision_frames([_frame(_rot([0.2, 1.0, -0.4], 0.8), c)])
        assert s.collision_form() == 3, s.collision_form()
else:
    s.set_collision_shapes([pkg.SHAPE["SPHERE"]], [[*c, R]])
s.keep_z(False)
s.initialize()
x0 = s.m_x.reshape(-1, 3)
in_box = (np.abs(x0 - c) < R).all(1).sum()
in_ball = (np.linalg.norm(x0 - c, axis=1) < R).sum()
s.step(iters); s.sync()
t0 = time.perf_counter()
for _ in range(frames):
    s.step(iters)
s.sync()
dt = time.perf_counter() - t0
print("%s: %d nodes, %d in the obstacle's box (%.1f %%), %d inside the ball; %.3f ms per ADMM iteration (wall, %d frames x %d)"
      % (mode, n, in_box, 100.0 * in_box / n, in_ball, 1e3 * dt / (frames * iters), frames, iters))
