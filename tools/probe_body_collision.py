#!/usr/bin/env python3
"""The cost of body surfaces (System.add_body_surface) on the MI355X, for DESIGN section 3:
  update    one NH bar of 32x32x163 cells (1.0 M tets) with its own boundary surface (46 k triangles) on the list next to a floor:
            the frame-start update's kernels (mesh_gather / check / volume / vertex_normal / slot / refit) per frame
  collide   two NH bars of 16x16x163 cells (255 k tets each) overlapping by half their width, each with its surface on the list:
            project_collision_mesh_kernel per ADMM iteration
Host wall time per frame is printed as JSON; the per-kernel split comes from one run under
  timeout -k 10 900 rocprofv3 --kernel-trace --stats -- python tools/probe_body_collision.py
usage: probe_body_collision.py [frames=5] [iters=10]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
mg = pkg.meshgen
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 5
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10


def scene(bars):
    xs, ts, n0 = [], [], 0
    s = pkg.System(device_id=0)
    s.set_timestep(0.02)
    for (nx, ny, nz), off in bars:
        x, t = mg.bar(nx, ny, nz)
        xs.append(x + np.asarray(off)); ts.append(t + n0); n0 += len(x)
    x, t = np.concatenate(xs), np.concatenate(ts).astype(np.int32)
    s.add_nodes(x.ravel(), np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3))
    s.add_forces(pkg.KIND["TET_NH"], t, [1e5, 1e5, 5])
    s.add_forces(pkg.KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity([0.0, -9.8, 0.0])
    ty, par, n0, ntri = [pkg.SHAPE["FLOOR"]], [[0.0, -0.5, 0.0, 0.0]], 0, []
    for xb, tb in zip(xs, ts):
        F = mg.tet_surface(tb - n0)
        mid = s.add_body_surface(n0, len(xb), F + n0)
        ty.append(pkg.SHAPE["MESH"]); par.append([0.0, 0.0, 0.0, mid]); ntri.append(len(F)); n0 += len(xb)
    s.set_collision_shapes(ty, par)
    s.initialize()
    return s, len(t), ntri


out = {}
for name, bars in (("update", [((32, 32, 163), (0, 0, 0))]), ("collide", [((16, 16, 163), (0, 0, 0)), ((16, 16, 163), (0.4, 0, 0))])):
    s, ntet, ntri = scene(bars)
    s.step(iters); s.sync()
    ts = []
    for f in range(frames):
        t0 = time.perf_counter()
        s.step(iters); s.sync()
        ts.append(time.perf_counter() - t0)
    st = s.body_surface_status(0)
    out[name] = dict(tets=ntet, surface_tris=ntri, frames=frames, iters=iters, frame_ms_median=round(1e3 * float(np.median(ts)), 3), status=st)
    del s
print(json.dumps({"probe": "body_collision", **out}))
