"""What rigid attachments cost a frame: tools/probe_rigid.py's bar (default 8 x 8 x 40 cells: 15 360 Neo-Hookean tets, 3 321 nodes) anchored
at one end, one collision element per node, contact attribution on, a sphere registered as a rigid body under gravity 1 mm above its
top, and the nodes of the bar's free end as a moving anchor batch -- the same frames with that batch left unattached and with it
attached to the sphere (admm_hip_attach_anchors: per frame attach_targets_kernel behind the pose launch, attach_partial_kernel and
attach_reduce_kernel before the bodies' integration).  Prints the wall time per frame of both, synchronised once at the end; the first
frames (graph capture) are left out.

    timeout -k 10 300 python tools/probe_attach.py [nx ny nz]

The numbers are a report, nothing is asserted."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def scene(pkg, attached, nx, ny, nz):
    mg = pkg.meshgen
    x, tets = mg.bar(nx, ny, nz)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    end = np.flatnonzero(np.abs(x[:, 2] - 0.05 * nz) < 1e-12).astype(np.int32)
    s = pkg.System(device_id=0)
    s.set_timestep(0.02)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(pkg.KIND["TET_NH"], tets, [1e5, 1e5, 5])
    s.add_forces(pkg.KIND["ANCHOR"], mg.bar_anchor_nodes(nx, ny), [1000.0, 1.0])
    batch = s.add_forces(pkg.KIND["ANCHOR"], end, [1000.0, 1.0], targets=x[end])
    s.add_forces(pkg.KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity((0.0, -9.8, 0.0))
    r = 0.1
    c = [0.05 * nx / 2, 0.05 * ny + r + 0.001, 0.05 * nz / 2]
    s.set_collision_shapes([pkg.SHAPE["SPHERE"]], [c + [r]])
    s.enable_contact_attribution(True)
    M = 0.25 * float(m.sum())
    body = s.add_rigid_body(0, M, [0.4 * M * r * r * d for d in (1, 0, 0, 1, 0, 1)], c, (0.0, -9.8, 0.0))
    if attached:
        s.attach_anchors(batch, body)
    s.initialize()
    return s, len(x), len(tets), len(end)


def main():
    pkg = load_package()
    dims = [int(a) for a in sys.argv[1:4]] if len(sys.argv) >= 4 else [8, 8, 40]
    warm, frames, iters = 5, 40, 10
    for attached in (False, True):
        s, n, nt, ne = scene(pkg, attached, *dims)
        for _ in range(warm):
            s.step(iters)
        s.sync()
        t0 = time.perf_counter()
        for _ in range(frames):
            s.step(iters)
        s.sync()
        ms = 1e3 * (time.perf_counter() - t0) / frames
        r = s.rigid_state()[0]
        Fa, Ta, na = s.attachment_load()
        print("%s: %d nodes, %d tets, %d anchors on the free end, %d frames x %d iterations: %.3f ms per frame; the sphere's centre y %.4f, %d contacts, "
              "%d attached elements active, carried F_y %.3g N" % ("attached  " if attached else "unattached", n, nt, ne, frames, iters, ms, r.c[1], r.count, int(na[0]), Fa[0][1]))
        del s


if __name__ == "__main__":
    main()
