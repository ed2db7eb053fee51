"""Deforming closed triangle-mesh obstacles: admm_hip_mesh_set_vertices (Mesh.set_vertices) on the host and
admm_hip_update_collision_mesh (System.update_collision_mesh) in a context -- the host query of a deformed mesh against the numpy brute
force and against a mesh created from the deformed vertices, refusals that leave the mesh as it was, and on the GPU: the device update
bit for bit against the host one over chains of updates, refusals on the device, a scene whose obstacle grows and turns between frames
under every launch mode and in two subtree shards, and the class API's CollisionMesh::set_vertices against a host-projected subclass.

Deformations: ico5 scaled anisotropically and translated; the cube rigidly rotated (sharp features: new edge and corner normals); the
torus twisted about its axis by a growing angle, then rotated by 90 degrees (loose refit boxes); ico5 with radial bumps (non-convex)."""

import threading

import numpy as np
import pytest

from checkers import KIND
from test_collision_mesh import mesh, brute_force, _points_system, _device_project, _bar_scene, _run, _np_floor, _np_sphere, \
    _scene_mesh_input

MESH = 3
FLOOR, SPHERE = 0, 1
ADMM_ERR_ARG = 1


# ---------------------------------------------------------------------------------------------------------------------------------
# deformations: deform(name, s) -> (base mesh, vertices at strength s); s = 1, 2, 3 make a chain of updates
# ---------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _aniso(V, s):
    return V * (1.0 + 0.1 * s * np.array([3.0, -2.0, 1.0])) + 0.05 * s * np.array([1.0, -2.0, 3.0])


def _cube_rot(V, s):
    c = np.array([0.5, 0.5, 0.5])
    return (V - c) @ _rot([1.0, 2.0, 0.5], np.radians(37.0) * s / 3.0).T + c


def _torus_twist(V, s):
    a = 0.6 * s * V[:, 2] / 0.35                                   # twist about z: the angle grows with the height
    ca, sa = np.cos(a), np.sin(a)
    W = np.stack([ca * V[:, 0] - sa * V[:, 1], sa * V[:, 0] + ca * V[:, 1], V[:, 2]], 1)
    return W @ _rot([1.0, 0.0, 0.0], np.radians(90.0) * s / 3.0).T


def _bumps(V, s):
    r = np.linalg.norm(V, axis=1)
    th = np.arctan2(V[:, 1], V[:, 0])
    ph = np.arccos(np.clip(V[:, 2] / r, -1, 1))
    return V * (1.0 + 0.15 * s / 3.0 * np.sin(5 * th) * np.sin(3 * ph))[:, None]


DEFORM = {"ico5_aniso": ("ico5", _aniso), "cube_rot37": ("cube", _cube_rot), "torus_twist": ("torus", _torus_twist),
          "ico5_bumps": ("ico5", _bumps)}


def deform(name, s):
    base, fn = DEFORM[name]
    V, F = mesh(base)
    return V, F, np.ascontiguousarray(fn(V, s))


def points(W, F, seed=0, n_box=4000):
    """query points of the (deformed) mesh: at vertices, on edges, just off the faces on both sides, far away, around and inside"""
    rng = np.random.default_rng(seed)
    lo, hi = W.min(0), W.max(0)
    scale = np.linalg.norm(hi - lo)
    fe = F[rng.choice(len(F), min(len(F), 1000), replace=False)]
    s = rng.uniform(0, 1, size=(len(fe), 1))
    cen = W[fe].mean(1)
    nrm = np.cross(W[fe[:, 1]] - W[fe[:, 0]], W[fe[:, 2]] - W[fe[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    parts = [W[rng.choice(len(W), min(len(W), 1000), replace=False)], W[fe[:, 0]] * (1 - s) + W[fe[:, 1]] * s,
             cen + 1e-3 * scale * nrm, cen - 1e-3 * scale * nrm, 0.5 * (lo + hi) + d * scale * rng.uniform(2, 5, size=(len(d), 1)),
             rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n_box, 3))]
    return np.ascontiguousarray(np.concatenate(parts)), scale


def winding_inside(V, F, P, chunk=128):
    """generalised winding number > 1/2 (solid angles of van Oosterom & Strackee)"""
    w = np.zeros(len(P))
    A0, B0, C0 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        a, b, c = A0[None] - p, B0[None] - p, C0[None] - p
        la, lb, lc = (np.linalg.norm(q, axis=2) for q in (a, b, c))
        det = np.einsum("pij,pij->pi", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("pij,pij->pi", a, b) * lc + np.einsum("pij,pij->pi", b, c) * la + np.einsum("pij,pij->pi", c, a) * lb
        w[s:s + chunk] = 2 * np.arctan2(det, den).sum(1) / (4 * np.pi)
    return w > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DEFORM))
def test_deformed_query_vs_brute_force_and_fresh_mesh(pkg, name):
    V, F, W = deform(name, 3)
    m = pkg.Mesh(V, F)
    for s in (1, 2, 3):                                                          # a chain of updates
        m.set_vertices(deform(name, s)[2])
    P, scale = points(W, F)
    t = np.array([0.25, -0.5, 1.0])
    proj, sd = m.query(P + t, t)
    pnp, d2, tri = brute_force(W, F, P)
    err = np.abs(proj - t - pnp).max()
    assert err <= 1e-12 * scale, (name, err)
    assert np.allclose(np.abs(sd), np.sqrt(d2), rtol=0, atol=1e-12 * scale)
    far = np.nonzero(np.sqrt(d2) > 1e-12)[0]
    far = far[np.random.default_rng(1).choice(len(far), min(len(far), 3000), replace=False)]
    ins = winding_inside(W, F, P[far])
    bad = np.nonzero((sd[far] > 0) != ins)[0]
    assert bad.size == 0, (name, bad[:10], P[far][bad[:3]])
    assert 0 < ins.sum() < len(far)                                               # both sides are sampled
    # a mesh created from the deformed vertices: the same closest points bit for bit, the same side away from the surface
    fp, fsd = pkg.Mesh(W, F).query(P + t, t)
    assert np.array_equal(proj, fp), (name, np.abs(proj - fp).max())
    sure = np.abs(fsd) > 1e-9
    assert np.array_equal(sd[sure] > 0, fsd[sure] > 0)
    # the boxes were refit: the root box is the deformed mesh's
    inf = m.info()
    assert np.array_equal(inf["lo"], W.min(0)) and np.array_equal(inf["hi"], W.max(0))


def test_refused_updates_leave_the_mesh_as_it_was(pkg):
    V, F = mesh("ico5")
    m = pkg.Mesh(V, F)
    m.set_vertices(_aniso(V, 1))
    P, _ = points(_aniso(V, 1), F, n_box=2000)
    before = m.query(P)

    def refused(W, *words):
        with pytest.raises(pkg.AdmmHipError) as e:
            m.set_vertices(W)
        for w in words:
            assert w in str(e.value), str(e.value)
        after = m.query(P)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        return str(e.value)

    refused(V[:-1], "%d vertices given" % (len(V) - 1), "has %d" % len(V))       # wrong nv
    Vn = V.copy(); Vn[F[7, 1], 2] = np.nan                                         # a NaN vertex: the lowest triangle using it is named
    refused(Vn, "triangle %d" % np.nonzero((F == F[7, 1]).any(1))[0].min(), "not finite")
    a, b = F[100, 0], F[100, 1]                                                    # one vertex moved onto a neighbour
    Vz = V.copy(); Vz[a] = V[b]
    lowest = np.nonzero((F == a).any(1) & (F == b).any(1))[0].min()
    refused(Vz, "triangle %d " % lowest, "degenerate", "zero area")
    refused(V * np.array([-1.0, 1.0, 1.0]), "non-positive volume")                 # the mirror image
    m.set_vertices(_aniso(V, 2))                                                  # and an accepted update still works
    assert not np.array_equal(m.query(P)[0], before[0])


@pytest.mark.parametrize("name", ["cube", "torus", "ico5"])
def test_update_to_creation_vertices_is_bit_identical(pkg, name):
    V, F = mesh(name)
    P, _ = points(V, F)
    m = pkg.Mesh(V, F)
    a = m.query(P)
    m.set_vertices(V)
    b = m.query(P)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(np.abs(a[1]), np.abs(b[1]))
    sure = np.abs(a[1]) > 1e-9
    assert np.array_equal(a[1][sure], b[1][sure])


def test_context_update_before_initialize_host_only(pkg):
    """a host-only context takes the update into its copy; a refusal names the mesh and the triangle"""
    V, F = mesh("cube")
    s = pkg.System(device_id=-1)
    x = np.random.default_rng(0).uniform(-1, 2, size=(40, 3))
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(40, dtype=np.int32), [32.0])
    mid = s.add_collision_mesh(V, F)
    s.update_collision_mesh(mid, _cube_rot(V, 3))
    with pytest.raises(pkg.AdmmHipError) as e:
        s.update_collision_mesh(mid + 1, V)
    assert "mesh_id 1" in str(e.value)
    Vz = V.copy(); Vz[F[4, 0]] = V[F[4, 1]]
    with pytest.raises(pkg.AdmmHipError) as e:
        s.update_collision_mesh(mid, Vz)
    assert "error 1" in str(e.value) and "collision mesh 0: triangle" in str(e.value) and "degenerate" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _host_want(m, P, t):
    proj, sd = m.query(P, t)
    return np.where((sd > 0)[:, None], proj, P)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEFORM))
def test_device_update_equals_host_update(pkg, name):
    V, F, W3 = deform(name, 3)
    chain = [deform(name, s)[2] for s in (1, 2, 3)]
    lo = np.min([W.min(0) for W in chain + [V]], 0); hi = np.max([W.max(0) for W in chain + [V]], 0)
    rng = np.random.default_rng(3)
    P0 = np.concatenate([points(W, F, seed=k)[0] for k, W in enumerate(chain)] + [rng.uniform(lo, hi, size=(4000, 3))])
    t = np.array([0.1, 0.2, -0.3])
    P = np.ascontiguousarray(P0 + t)
    host = pkg.Mesh(V, F)
    s, b = _points_system(pkg, P, [MESH], [[*t, 0]], [(V, F)])
    cy, c, R = float(t[1] - 0.2), np.array([0.3, 0.0, 0.1]) + t, 0.45
    s2, b2 = _points_system(pkg, P, [FLOOR, MESH, SPHERE], [[0, cy, 0, 0], [*t, 0], [*c, R]], [(V, F)])
    for k, W in enumerate(chain):
        host.set_vertices(W)
        s.update_collision_mesh(0, W)
        s2.update_collision_mesh(0, W)
        z = _device_project(s, b, P)
        want = _host_want(host, P, t)
        assert (want != P).any(1).sum() > 500
        assert np.array_equal(z, want), (name, k, np.abs(z - want).max(), np.count_nonzero((z != want).any(1)))
        # [floor, mesh, sphere]: the deformed mesh composed with the analytic shapes in list order
        z2 = _device_project(s2, b2, P)
        p = _host_want(host, _np_floor(P, cy), t)
        p = _np_sphere(p, c, R)
        assert np.array_equal(z2, p), (name, k, np.abs(z2 - p).max())


@pytest.mark.gpu
def test_device_refusal_and_update_before_initialize(pkg):
    V, F = mesh("ico5")
    W1, W2 = _bumps(V, 2), _aniso(V, 1)
    P = np.ascontiguousarray(np.concatenate([points(W, F, seed=k)[0] for k, W in enumerate((V, W1, W2))]))
    t = np.zeros(3)
    host = pkg.Mesh(V, F)
    # an update before initialize goes into the context's copy: the same as the host update
    s = pkg.System(device_id=0)
    s.set_timestep(0.02)
    s.add_nodes(P.ravel(), np.ones(P.size))
    b = s.add_forces(KIND["COLLISION"], np.arange(len(P), dtype=np.int32), [32.0])
    mid = s.add_collision_mesh(V, F)
    s.set_collision_shapes([MESH], [[*t, mid]])
    s.update_collision_mesh(mid, W1)
    s.initialize()
    host.set_vertices(W1)
    z1 = _device_project(s, b, P)
    assert np.array_equal(z1, _host_want(host, P, t))
    # refusals after initialize: ADMM_ERR_ARG, the projection bitwise as before
    a, c = F[100, 0], F[100, 1]
    Vz = W2.copy(); Vz[a] = W2[c]
    lowest = np.nonzero((F == a).any(1) & (F == c).any(1))[0].min()
    Vn = W2.copy(); Vn[F[9, 2], 0] = np.inf
    for bad, words in ((Vz, ["triangle %d " % lowest, "degenerate"]), (Vn, ["not finite"]), (W2 * np.array([1.0, -1.0, 1.0]), ["volume"]),
                       (W2[:-3], ["vertices given"])):
        with pytest.raises(pkg.AdmmHipError) as e:
            s.update_collision_mesh(mid, bad)
        msg = str(e.value)
        assert ("error %d" % ADMM_ERR_ARG) in msg and "collision mesh 0" in msg, msg
        for w in words:
            assert w in msg, msg
        assert np.array_equal(_device_project(s, b, P), z1)
    # the same refusals on the host object, with the same message
    with pytest.raises(pkg.AdmmHipError) as e:
        host.set_vertices(Vz)
    assert ("triangle %d " % lowest) in str(e.value)
    s.update_collision_mesh(mid, W2)
    host.set_vertices(W2)
    assert np.array_equal(_device_project(s, b, P), _host_want(host, P, t))


def _growing(f, V):
    """ico5 of radius 0.3 growing 1 % a frame, turning 4 degrees a frame about a tilted axis"""
    return np.ascontiguousarray((V * 0.3 * 1.01 ** f) @ _rot([0.3, 1.0, 0.2], np.radians(4.0) * f).T)


def _deform_scene(pkg, **kw):
    V, F = mesh("ico5")
    c = np.array([0.15, -0.34, 0.96])                   # under the bar's free end
    sh = lambda f: ([FLOOR, MESH], [[0, -0.6, 0, 0], [*c, 0]])
    s = _bar_scene(pkg, [(_growing(0, V), F)], sh, **kw)
    return s, V, c


def _deform_frames(s, V, frames, iters=10):
    xs = []
    for f in range(frames):
        if f:
            s.update_collision_mesh(0, _growing(f, V))
        s.step(iters)
        xs.append(s.m_x.copy())
    return xs


@pytest.mark.gpu
def test_deforming_obstacle_scene_launch_modes(pkg, monkeypatch):
    frames = 12
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {"ADMM_HIP_LOCAL_MULTI": "0"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s, V, c = _deform_scene(pkg)
        s.initialize()
        xs = _deform_frames(s, V, frames)
        res[tuple(env.items())] = (xs, s.graph_state())
    keys = list(res)
    for k in keys[1:]:
        for f in range(frames):
            assert np.array_equal(res[keys[0]][0][f], res[k][0][f]), (k, f)
    g = res[keys[0]][1]
    assert g["iter_graph"] or g["frame_graph_iters"] > 0                           # GRAPH=1 replayed graphs across the updates
    R = 0.3 * 1.01 ** (frames - 1)
    r = np.linalg.norm(res[keys[0]][0][-1].reshape(-1, 3) - c, axis=1)
    print("deforming scene: radius %.4f, closest node %.4f, %d nodes within 1 cm of the surface" % (R, r.min(), int((np.abs(r - R) < 0.01).sum())))
    assert r.min() > R - 0.01 and (np.abs(r - R) < 0.01).any()


@pytest.mark.gpu
def test_deforming_obstacle_scene_two_subtree_shards(pkg, monkeypatch):
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    frames = 8
    ref, V, c = _deform_scene(pkg)
    ref.initialize()
    shards = [_deform_scene(pkg, rank=r, world=2, mode="subtree")[0] for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    assert sum(s.info()["n_elems_local"] for s in shards) == ref.info()["n_elems_total"]
    out, errs = [None, None], []

    def run(r):
        try:
            out[r] = (_deform_frames(shards[r], V, frames), shards[r].m_v.copy())      # every rank applies the same updates
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join(timeout=300)
    assert not errs, errs
    refx = _deform_frames(ref, V, frames)
    for r in range(2):
        xs, vs = out[r]
        for f in range(frames):
            assert np.abs(xs[f] - refx[f]).max() < 1e-9, (r, f, np.abs(xs[f] - refx[f]).max())
        assert np.array_equal(xs[-1], out[0][0][-1]) and np.array_equal(vs, out[0][1])
    R = 0.3 * 1.01 ** (frames - 1)
    r = np.linalg.norm(refx[-1].reshape(-1, 3) - c, axis=1)
    assert (r < R + 0.01).any()                                                     # contact happened


@pytest.mark.gpu
def test_class_api_deforming_mesh_vs_host_projected(pkg, tmp_path):
    import subprocess
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_mesh_deform", pkg)
    inp = str(tmp_path / "in.bin")
    V, F, x, c0 = _scene_mesh_input(pkg, inp)
    frames, iters, n = 30, 10, len(x)
    out = {}
    for mode in range(4):
        o = str(tmp_path / ("out%d.bin" % mode))
        r = subprocess.run([exe, str(mode), inp, o, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (mode, r.stdout, r.stderr)
        out[mode] = np.fromfile(o).reshape(frames, n, 3)
    control = np.abs(out[0] - out[1]).max()
    diff = np.abs(out[2] - out[3]).max()
    if control == 0.0:
        print("class API (deforming): the control is bitwise equal, so the mesh pair must be too: max diff %g" % diff)
        assert diff == 0.0
    else:
        print("class API (deforming): the control differs by %g, the mesh pair by %g" % (control, diff))
        assert diff <= control
    # the obstacle really deformed under the plate: the deformed mesh's query, frame by frame (the scene's own deformation)
    m = pkg.Mesh(V, F)
    touched = np.zeros(n, bool)
    for f in range(frames):
        m.set_vertices(_scene_deform(V, f))
        _, sd = m.query(out[2][f], c0[:3])
        touched |= sd > -5e-3
    print("class API (deforming): %d of %d nodes (%.1f %%) reached the obstacle" % (touched.sum(), n, 100.0 * touched.mean()))
    assert touched.mean() >= 0.05
    assert not np.array_equal(out[2][-1], _static_run(exe, inp, tmp_path, frames, iters, n))      # the deformation mattered


def _scene_deform(V, f):
    """tests/cpp/scene_mesh_deform.cpp's deformation of frame f: scaled by 1 + 0.004 f, turned 3 degrees a frame about y"""
    a = np.radians(3.0) * f
    s = 1.0 + 0.004 * f
    ca, sa = np.cos(a), np.sin(a)
    W = V * s
    return np.stack([ca * W[:, 0] + sa * W[:, 2], W[:, 1], -sa * W[:, 0] + ca * W[:, 2]], 1)


def _static_run(exe, inp, tmp_path, frames, iters, n):
    import subprocess
    o = str(tmp_path / "static.bin")
    r = subprocess.run([exe, "4", inp, o, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return np.fromfile(o).reshape(frames, n, 3)[-1]
