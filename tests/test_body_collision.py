"""Body surfaces: closed meshes of simulated nodes (System.add_body_surface, admm_hip_add_body_surface) that the device rebuilds from the
frame-start x at every step, and mesh owners (set_collision_mesh_owner) whose nodes skip their own mesh.

CPU (host-only contexts): every refusal, meshgen.tet_surface on the bar and the shipped dillo / bunny tet meshes, and the vertex order
and triangle numbering of a registered body surface against Mesh(x[sorted nodes], renumbered tris).
GPU: the frame-start update bit for bit against the host-driven route that exists without it (plain obstacles with the same owners,
update_collision_mesh with x[surface nodes] before every step) under every launch mode and in two subtree shards; a body's own
surface is ignored; contact between two bars against a control without surfaces; a refused frame keeps the last good surface; the
class API's CollisionBody reproduces the Python run."""

import os
import threading

import numpy as np
import pytest

from checkers import KIND

MESH, FLOOR = 3, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADMM_ERR_ARG, ADMM_ERR_STATE = 1, 3
DT, FLOOR_Y = 0.02, -0.3


def _roty(x):
    """a quarter turn about y (orientation kept): the bar's long axis z becomes x"""
    return np.stack([x[:, 2], x[:, 1], -x[:, 0]], 1)


def _two_bars(pkg, drop=True):
    """bar A (3x3x12 cells of 5 cm along z, anchored at z = 0 when `drop`) and bar B (3x3x8 cells, turned to lie along x) above
    A's free half; without `drop` both bars are free, side by side along x, for a push at each other.
    -> (x [n][3], tets, anchors, masses, node count of A, (surface of A, surface of B))"""
    mg = pkg.meshgen
    xa, ta = mg.bar(3, 3, 12)
    xb, tb = mg.bar(3, 3, 8)
    if drop:
        xb = _roty(xb) + np.array([-0.125, 0.2, 0.5])
        anch = mg.bar_anchor_nodes(3, 3)
    else:
        xb = xb + np.array([0.25, 0.0, 0.1])
        anch = np.zeros(0, np.int32)
    na = len(xa)
    x = np.concatenate([xa, xb])
    tets = np.concatenate([ta, tb + na]).astype(np.int32)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    sa = mg.tet_surface(ta, xa)
    sb = (mg.tet_surface(tb, xb) + na).astype(np.int32)
    return x, tets, anch.astype(np.int32), m, na, (sa, sb)


def _system(pkg, scene, kind="TET_NH", gravity=True, device_id=0, rank=0, world=1, mode=None):
    x, tets, anch, m, na, _ = scene
    s = pkg.System(device_id=device_id)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND[kind], tets, [1e5, 1e5, 5] if kind in ("TET_NH", "TET_STVK") else [2e4])
    if len(anch):
        s.add_forces(KIND["ANCHOR"], anch, [1000.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    if gravity:
        s.add_gravity([0.0, -9.8, 0.0])
    if world > 1:
        s.set_shard(rank, world)
        if mode:
            s.set_shard_mode(mode)
    s.n_x = len(x)
    return s


def _surface_nodes(tris):
    return np.unique(np.asarray(tris).ravel())


def _renumber(tris):
    nodes = _surface_nodes(tris)
    return nodes, np.searchsorted(nodes, tris).astype(np.int32)


def _with_bodies(pkg, scene, floor=True, **kw):
    """route 1: both surfaces registered with add_body_surface"""
    x, _, _, _, na, (sa, sb) = scene
    s = _system(pkg, scene, **kw)
    ia = s.add_body_surface(0, na, sa)
    ib = s.add_body_surface(na, len(x) - na, sb)
    ty, par = [MESH, MESH], [[0, 0, 0, ia], [0, 0, 0, ib]]
    if floor:
        ty, par = [FLOOR] + ty, [[0, FLOOR_Y, 0, 0]] + par
    s.set_collision_shapes(ty, par)
    s.bodies = [ia, ib]
    return s


def _with_obstacles(pkg, scene, floor=True, **kw):
    """route 2 (exists without the feature's device step): the same meshes as plain obstacles created from the same x0 in the same
    vertex order, with the same owners; the caller hands x[surface nodes] to update_collision_mesh before every step"""
    x, _, _, _, na, (sa, sb) = scene
    s = _system(pkg, scene, **kw)
    s.obst = []
    for tris, first, cnt in ((sa, 0, na), (sb, na, len(x) - na)):
        nodes, loc = _renumber(tris)
        mid = s.add_collision_mesh(x[nodes], loc)
        s.set_collision_mesh_owner(mid, first, cnt)
        s.obst.append((mid, nodes))
    ty, par = [MESH, MESH], [[0, 0, 0, s.obst[0][0]], [0, 0, 0, s.obst[1][0]]]
    if floor:
        ty, par = [FLOOR] + ty, [[0, FLOOR_Y, 0, 0]] + par
    s.set_collision_shapes(ty, par)
    return s


def _frames(s, frames, iters=10, host_updates=False):
    out = []
    for f in range(frames):
        if host_updates:
            X = s.m_x.reshape(-1, 3)
            for mid, nodes in s.obst:
                s.update_collision_mesh(mid, X[nodes])
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


def _depth(pkg, x, tris, pts):
    """the deepest of pts inside the closed surface (x, tris): the host query's signed distance (> 0 inside), 0 if none is inside"""
    nodes, loc = _renumber(tris)
    _, sd = pkg.Mesh(x[nodes], loc).query(pts)
    return max(0.0, float(sd.max()))


def _read_tetgen(name):
    base = os.path.join(ROOT, "tests", "golden", "scenes", name)
    X = np.loadtxt(base + ".node", skiprows=1, comments="#")[:, 1:4]
    E = np.loadtxt(base + ".ele", skiprows=1, comments="#", dtype=np.int64)[:, 1:5]
    return X, E


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(pkg, s, rc, words, fn, *args):
    with pytest.raises(pkg.AdmmHipError) as e:
        fn(*args)
    msg = str(e.value)
    assert ("error %d" % rc) in msg or ("code %d" % rc) in msg or (" %d:" % rc) in msg or (" %d " % rc) in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_refusals(pkg):
    scene = _two_bars(pkg)
    x, _, _, _, na, (sa, sb) = scene
    n = len(x)
    s = _system(pkg, scene, device_id=-1)
    # node ids outside the range, a range outside the nodes
    _refused(pkg, s, ADMM_ERR_ARG, ["outside"], s.add_body_surface, 0, na - 1, sa)
    _refused(pkg, s, ADMM_ERR_ARG, ["outside"], s.add_body_surface, na, n - na, sa)
    _refused(pkg, s, ADMM_ERR_ARG, ["not inside"], s.add_body_surface, na, n - na + 1, sb)
    _refused(pkg, s, ADMM_ERR_ARG, ["not inside"], s.add_body_surface, -1, na, sa)
    # open, non-manifold, inward-oriented surfaces (admm_hip_mesh_create's messages)
    _refused(pkg, s, ADMM_ERR_ARG, ["body surface", "open"], s.add_body_surface, 0, na, sa[1:])
    _refused(pkg, s, ADMM_ERR_ARG, ["body surface", "not edge-manifold"], s.add_body_surface, 0, na, np.concatenate([sa, sa[:1]]))
    _refused(pkg, s, ADMM_ERR_ARG, ["body surface", "non-positive volume"], s.add_body_surface, 0, na, sa[:, [0, 2, 1]])
    ia = s.add_body_surface(0, na, sa)
    # overlapping owner ranges; equal ones are fine
    nodes, loc = _renumber(sb)
    mid = s.add_collision_mesh(x[nodes], loc)
    _refused(pkg, s, ADMM_ERR_ARG, ["overlaps"], s.set_collision_mesh_owner, mid, 1, na)
    _refused(pkg, s, ADMM_ERR_ARG, ["overlaps"], s.add_body_surface, na - 2, n - na + 2, sb)
    s.set_collision_mesh_owner(mid, 0, na)
    s.set_collision_mesh_owner(mid, 0, 0)                         # cleared
    _refused(pkg, s, ADMM_ERR_ARG, ["not a registered mesh"], s.set_collision_mesh_owner, 7, 0, na)
    ib = s.add_body_surface(na, n - na, sb)
    # update_collision_mesh on a body surface
    _refused(pkg, s, ADMM_ERR_ARG, ["follows its nodes"], s.update_collision_mesh, ia, x[_surface_nodes(sa)])
    # a body surface named with a translation (the list names registered meshes only, so set_collision_shapes sees both)
    _refused(pkg, s, ADMM_ERR_ARG, ["body surface", "translation"], s.set_collision_shapes, [FLOOR, MESH], [[0, -1, 0, 0], [0, 0.1, 0, ib]])
    s.set_collision_shapes([FLOOR, MESH, MESH], [[0, -1, 0, 0], [0, 0, 0, ia], [0.5, 0, 0, mid]])      # an obstacle may move
    # phases
    _refused(pkg, s, ADMM_ERR_STATE, ["before finalize"], s.body_surface_status, ia)
    s.initialize()
    assert s.body_surface_status(ia) == dict(updated=0, refused=0, last_bad_tri=-1)
    _refused(pkg, s, ADMM_ERR_ARG, ["not a body surface"], s.body_surface_status, mid)
    _refused(pkg, s, ADMM_ERR_STATE, ["before finalize"], s.add_body_surface, 0, na, sa)
    _refused(pkg, s, ADMM_ERR_STATE, ["before finalize"], s.set_collision_mesh_owner, mid, 0, na)


def test_tet_surface_bar_and_shipped_meshes(pkg):
    mg = pkg.meshgen
    for nx, ny, nz in ((1, 1, 1), (2, 3, 4), (3, 3, 12)):
        x, t = mg.bar(nx, ny, nz)
        F = mg.tet_surface(t)
        assert F.dtype == np.int32 and len(F) == 4 * (nx * ny + ny * nz + nx * nz)     # two triangles per boundary square
        assert np.array_equal(F, mg.tet_surface(t, x))                                 # bar tets are positively oriented
        nodes, loc = _renumber(F)
        info = pkg.Mesh(x[nodes], loc).info()
        assert info["n_tris"] == len(F)
        assert np.allclose(info["lo"], 0) and np.allclose(info["hi"], [0.05 * nx, 0.05 * ny, 0.05 * nz])
    for name in ("poordillo/dillo919", "bunnyexpand/bunny_1124"):
        X, E = _read_tetgen(name)
        F = mg.tet_surface(E, X)
        assert np.array_equal(F, mg.tet_surface(E))                                    # (positively oriented too)
        nodes, loc = _renumber(F)
        m = pkg.Mesh(X[nodes], loc)                                                   # closed, manifold, outward
        _, sd = m.query(X[E].mean(1)[::7])                                            # tet centroids are inside
        assert (sd > 0).all(), name
        edges = np.unique(np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1), axis=0)
        assert len(nodes) - len(edges) + len(F) == 2, name                            # a closed surface of genus 0


def test_body_surface_vertex_order_and_numbering(pkg):
    scene = _two_bars(pkg)
    x, _, _, _, na, (sa, sb) = scene
    s = _system(pkg, scene, device_id=-1)
    rng = np.random.default_rng(3)
    sb_rot = sb[:, [1, 2, 0]][rng.permutation(len(sb))]           # corners rotated, triangles shuffled: the order given is kept
    x1 = x + 0.001 * rng.standard_normal(x.shape)
    s.m_x = x1.ravel()                                              # the positions at registration are the current ones
    ia = s.add_body_surface(0, na, sa)
    ib = s.add_body_surface(na, len(x) - na, sb_rot)
    for mid, tris in ((ia, sa), (ib, sb_rot)):
        nodes, loc = _renumber(tris)
        want = pkg.Mesh(x1[nodes], loc)
        got = s.collision_mesh(mid)
        a, b = got.info(), want.info()
        assert a["n_tris"] == b["n_tris"] and a["n_nodes"] == b["n_nodes"] and a["depth"] == b["depth"]
        assert np.array_equal(a["lo"], b["lo"]) and np.array_equal(a["hi"], b["hi"])
        P = np.concatenate([x1[nodes] + 0.01 * rng.standard_normal((len(nodes), 3)), x1[rng.integers(0, len(x1), 400)]])
        pa, da = got.query(P)
        pb, db = want.query(P)
        assert np.array_equal(pa, pb) and np.array_equal(da, db)
        assert (da > 0).any() and (da < 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_same(a, b, what):
    for f, ((xa, va), (xb, vb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(va, vb), (what, f, np.abs(xa - xb).max())


@pytest.mark.gpu
def test_follow_equals_host_driven_launch_modes(pkg, monkeypatch):
    frames = 24
    scene = _two_bars(pkg)
    na = scene[4]
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        b = _with_bodies(pkg, scene); b.initialize()
        o = _with_obstacles(pkg, scene); o.initialize()
        rb, ro = _frames(b, frames), _frames(o, frames, host_updates=True)
        _assert_same(rb, ro, env)
        g = b.graph_state()
        print("launch mode %s: %s" % (env, g))
        if env.get("ADMM_HIP_GRAPH") == "0":
            assert not g["iter_graph"] and g["frame_graph_iters"] == 0
        elif env:
            assert g["iter_graph"] and g["frame_graph_iters"] == 0
        else:
            assert g["frame_graph_iters"] == 10
        assert b.body_surface_status(b.bodies[0]) == dict(updated=frames, refused=0, last_bad_tri=-1)
        res[tuple(env.items())] = rb
    keys = list(res)
    for k in keys[1:]:
        _assert_same(res[keys[0]], res[k], k)
    x = res[keys[0]][-1][0].reshape(-1, 3)
    print("follow: lowest B node y %.4f, A's highest node y %.4f" % (x[na:, 1].min(), x[:na, 1].max()))


@pytest.mark.gpu
def test_follow_equals_host_driven_two_subtree_shards(pkg, monkeypatch):
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    frames = 20
    scene = _two_bars(pkg)
    kw = dict(kind="TET_LINEAR")                 # (the existing two-shard mesh tests' material: no line search to amplify the shards' rounding)
    ref = _with_bodies(pkg, scene, **kw); ref.initialize()
    refx = _frames(ref, frames)
    out = {}
    for route in ("bodies", "obstacles"):
        make = _with_bodies if route == "bodies" else _with_obstacles
        shards = [make(pkg, scene, rank=r, world=2, mode="subtree", **kw) for r in range(2)]
        hooks = _thread_allreduce_hooks(2)
        for r, s in enumerate(shards):
            s.set_allreduce(hooks[r])
        pkg.initialize_together(shards)
        assert sum(s.info()["n_elems_local"] for s in shards) == ref.info()["n_elems_total"]
        res, errs = [None, None], []

        def run(r):
            try:
                res[r] = _frames(shards[r], frames, host_updates=route == "obstacles")
            except Exception as e:  # noqa: BLE001
                errs.append((r, e))
        th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join(timeout=300)
        assert not errs, errs
        _assert_same(res[0], res[1], (route, "rank 1 vs rank 0"))
        out[route] = res[0]
    _assert_same(out["bodies"], out["obstacles"], "two shards")
    for f in range(frames):
        d = np.abs(out["bodies"][f][0] - refx[f][0]).max()
        assert d < 1e-9, (f, d)


@pytest.mark.gpu
def test_own_surface_is_ignored(pkg):
    x, tets, anch, _, na, (sa, _) = _two_bars(pkg)
    ta = tets[np.all(tets < na, axis=1)]
    one = (x[:na], ta, anch, pkg.meshgen.lumped_tet_mass(x[:na], ta, 1000.0), na, None)
    floor = [0, FLOOR_Y + 0.25, 0, 0]
    a = _system(pkg, one)
    a.set_collision_shapes([FLOOR], [floor])
    b = _system(pkg, one)
    ia = b.add_body_surface(0, na, sa)
    b.set_collision_shapes([FLOOR, MESH], [floor, [0, 0, 0, ia]])
    a.initialize(); b.initialize()
    ra, rb = _frames(a, 20), _frames(b, 20)
    _assert_same(ra, rb, "own surface")
    assert ra[-1][0].reshape(-1, 3)[:, 1].min() < floor[1] + 1e-3                     # the bar reached the floor
    assert b.body_surface_status(ia)["updated"] == 20


def _contact(pkg, scene, bodies, frames, gravity):
    x, _, _, _, na, (sa, sb) = scene
    if bodies:
        s = _with_bodies(pkg, scene, gravity=gravity)
    else:
        s = _system(pkg, scene, gravity=gravity)
        s.set_collision_shapes([FLOOR], [[0, FLOOR_Y, 0, 0]])
    s.initialize()
    if not gravity:
        v = np.zeros_like(x)
        v[:na, 0], v[na:, 0] = 0.25, -0.25
        s.m_v = v.ravel()
    dab, dba, cen = [], [], []
    for f in range(frames):
        s.step(10)
        X = s.m_x.reshape(-1, 3)
        dab.append(_depth(pkg, X, sb, X[:na]))                                           # A's nodes inside B's frame-end surface
        dba.append(_depth(pkg, X, sa, X[na:]))
        cen.append(np.linalg.norm(X[na:].mean(0) - X[:na].mean(0)))
    return max(dab), max(dba), np.array(cen)


@pytest.mark.gpu
def test_contact_drop_and_push_against_control(pkg):
    """(a) B dropped across A, a cantilever over the floor; (b) two free bars pushed at each other at 0.25 m/s each, no gravity.  The
    deepest node of either bar inside the other's frame-end surface over 30 frames, with surfaces and without (the control).
    Measured on the MI355X (the same bits in two runs): (a) 0.0196 / 0.0167 m with surfaces, 0.0634 / 0.0689 m without; (b) 0.00105 /
    0.00107 m with surfaces, 0.0500 / 0.0500 m without (the deepest grid node of a 15 cm bar lies 5 cm inside), the centroids 0.240 m
    apart at the start, 0.149 at the closest, 0.166 at the end.  The surfaces are frozen for a frame, so a closing speed w lets nodes
    in by about w * dt before the next frame's surface pushes them out: at 1 m/s each (b) reached 0.048 m, hence the slower push.
    Bounds 0.025 m for (a) and 0.005 m for (b); each control must exceed twice its scene's bound (2.8x and 10x measured)."""
    frames = 30
    drop, push = _two_bars(pkg), _two_bars(pkg, drop=False)
    wa, ca = _contact(pkg, drop, True, frames, True), _contact(pkg, drop, False, frames, True)
    wb, cb = _contact(pkg, push, True, frames, False), _contact(pkg, push, False, frames, False)
    print("contact depths (m): drop with %.5f / %.5f, without %.5f / %.5f; push with %.5f / %.5f, without %.5f / %.5f" %
          (wa[0], wa[1], ca[0], ca[1], wb[0], wb[1], cb[0], cb[1]))
    print("push centroid distance: start %.4f, min %.4f, end %.4f" % (wb[2][0], wb[2].min(), wb[2][-1]))
    BOUND_A, BOUND_B = 0.025, 0.005
    assert max(wa[0], wa[1]) < BOUND_A and max(wb[0], wb[1]) < BOUND_B
    assert max(ca[0], ca[1]) > 2 * BOUND_A and max(cb[0], cb[1]) > 2 * BOUND_B
    assert wb[2][-1] > wb[2].min() + 1e-3                                                # the bars separate again


@pytest.mark.gpu
def test_refused_frame_keeps_the_last_good_surface(pkg):
    frames, bad = 14, 6
    scene = _two_bars(pkg)
    sb = scene[5][1]
    b = _with_bodies(pkg, scene, kind="TET_LINEAR"); b.initialize()
    o = _with_obstacles(pkg, scene, kind="TET_LINEAR"); o.initialize()
    t = sb[len(sb) // 2]                                           # the surface triangle of B whose third corner collapses onto its first
    rb, ro = [], []
    want_bad = None
    for f in range(frames):
        if f == bad:
            for s in (b, o):
                X = s.m_x.reshape(-1, 3).copy()
                X[t[2]] = X[t[0]]
                s.m_x = X.ravel()
            X = b.m_x.reshape(-1, 3)
            area2 = np.linalg.norm(np.cross(X[sb[:, 1]] - X[sb[:, 0]], X[sb[:, 2]] - X[sb[:, 0]]), axis=1)
            want_bad = int(np.flatnonzero(area2 == 0.0)[0])
            with pytest.raises(pkg.AdmmHipError):                  # the host-driven route is refused there and skips that update
                o.update_collision_mesh(o.obst[1][0], X[o.obst[1][1]])
            o.update_collision_mesh(o.obst[0][0], X[o.obst[0][1]])
        else:
            X = o.m_x.reshape(-1, 3)
            for mid, nodes in o.obst:
                o.update_collision_mesh(mid, X[nodes])
        b.step(10); o.step(10)
        rb.append((b.m_x.copy(), b.m_v.copy())); ro.append((o.m_x.copy(), o.m_v.copy()))
        st = b.body_surface_status(b.bodies[1])
        if f == bad:
            assert st == dict(updated=bad, refused=1, last_bad_tri=want_bad), st
        if f == bad + 1:
            assert st == dict(updated=bad + 1, refused=1, last_bad_tri=want_bad), st
    _assert_same(rb, ro, "refused frame")
    assert all(np.isfinite(xx).all() for xx, _ in rb)
    assert b.body_surface_status(b.bodies[0]) == dict(updated=frames, refused=0, last_bad_tri=-1)


@pytest.mark.gpu
def test_class_api_collision_body(pkg, tmp_path):
    import subprocess
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_bodies", pkg)
    scene = _two_bars(pkg)
    x, tets, anch, m, na, (sa, sb) = scene
    frames, iters = 20, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(tets), len(anch), na, len(sa), len(sb)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (tets, anch, sa, sb):
            a.astype(np.int32).tofile(f)
        np.array([FLOOR_Y, DT]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(outp).reshape(frames, 2, len(x) * 3)
    s = _with_bodies(pkg, scene); s.initialize()
    want = _frames(s, frames, iters)
    for f in range(frames):
        assert np.array_equal(got[f, 0], want[f][0]) and np.array_equal(got[f, 1], want[f][1]), (f, np.abs(got[f, 0] - want[f][0]).max())
