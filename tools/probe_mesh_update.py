#!/usr/bin/env python3
"""The cost of deforming a mesh obstacle between frames: System.update_collision_mesh (admm_hip_update_collision_mesh) on a level-7
icosphere (327 680 triangles, 163 842 vertices) registered with a small context, in host wall time per call -- the pageable H2D copy
of the vertices, the check stage and its 16-byte read-back, the commit stage and the per-level refit, the final sync.  Alternates two
deformed vertex sets so that every call really changes the mesh.  For the per-kernel split run it once under
  rocprofv3 --kernel-trace --stats -- python tools/probe_mesh_update.py
usage: probe_mesh_update.py [updates=50]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
from test_collision_mesh import icosphere  # noqa: E402

pkg = load_package()
n_upd = int(sys.argv[1]) if len(sys.argv) > 1 else 50
V, F = icosphere(7)
W = [np.ascontiguousarray(V * np.array([1.0 + 0.02 * k, 1.0 - 0.01 * k, 1.0])) for k in (1, 2)]
P = np.random.default_rng(0).uniform(-1.2, 1.2, size=(4096, 3))
s = pkg.System(device_id=0)
s.set_timestep(0.02)
s.add_nodes(P.ravel(), np.ones(P.size))
s.add_forces(pkg.KIND["COLLISION"], np.arange(len(P), dtype=np.int32), [32.0])
mid = s.add_collision_mesh(V, F)
s.set_collision_shapes([pkg.SHAPE["MESH"]], [[0.0, 0.0, 0.0, mid]])
s.initialize()
s.step(1)
s.sync()
for k in range(3):                                  # warm-up: first launches of the update kernels
    s.update_collision_mesh(mid, W[k % 2])
ts = []
for k in range(n_upd):
    t0 = time.perf_counter()
    s.update_collision_mesh(mid, W[k % 2])
    ts.append(time.perf_counter() - t0)
ts = np.array(ts) * 1e3
inf = pkg.Mesh(V, F).info()
print(json.dumps({"probe": "mesh_update", "n_tris": int(len(F)), "n_verts": int(len(V)), "bvh_depth": inf["depth"], "updates": n_upd,
                  "ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(ts.min()), 4), "ms_max": round(float(ts.max()), 4)}))
