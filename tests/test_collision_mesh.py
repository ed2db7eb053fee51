"""Closed triangle-mesh obstacles (ADMM_SHAPE_MESH): registration and its validation, the host query (admm_hip_mesh_query) against an
independent numpy brute force, the determinism of its tie rule, and on the GPU: the device query bit for bit against the host one,
mixed shape lists, the no-mesh path left as it was, launch modes and subtree shards.

The meshes are generated here with numpy: icospheres (levels 2, 5, 7), a unit cube (sharp edges and corners for the pseudo-normals),
a torus (non-convex, a hole inside its box)."""

import numpy as np
import pytest

from checkers import KIND

MESH = 3
FLOOR, SPHERE = 0, 1


# ---------------------------------------------------------------------------------------------------------------------------------
# mesh fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
def icosphere(level, radius=1.0):
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid = {}

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        nf = []
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    V = np.array(v) * radius
    F = np.array(f, dtype=np.int32)
    return orient(V, F)


def cube():
    V = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return orient(V, F)


def torus(R=1.0, r=0.35, nu=48, nv=24):
    u = np.arange(nu) * 2 * np.pi / nu
    w = np.arange(nv) * 2 * np.pi / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    V = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    F = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            F += [[a, b, c], [a, c, d]]
    return orient(V, np.array(F, dtype=np.int32))


def orient(V, F):
    """every triangle counter-clockwise seen from outside: the generators above orient all triangles alike, so one signed volume decides"""
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    if np.einsum("ij,ij->i", a, np.cross(b, c)).sum() < 0:
        F = F[:, [0, 2, 1]]
    return V, np.ascontiguousarray(F)


MESHES = {"cube": cube, "torus": torus, "ico2": lambda: icosphere(2), "ico5": lambda: icosphere(5), "ico7": lambda: icosphere(7)}
_cache = {}


def mesh(name):
    if name not in _cache:
        _cache[name] = MESHES[name]()
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# the sample of query points, the independent brute force
# ---------------------------------------------------------------------------------------------------------------------------------
def sample_points(name, n_min=10000, seed=0):
    V, F = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = V.min(0), V.max(0)
    scale = np.linalg.norm(hi - lo)
    cap = 2000
    parts = [V[rng.choice(len(V), min(len(V), cap), replace=False)]]                                 # exactly at vertices
    fe = F[rng.choice(len(F), min(len(F), cap), replace=False)]
    s = rng.uniform(0, 1, size=(len(fe), 1))
    parts.append(V[fe[:, 0]] * (1 - s) + V[fe[:, 1]] * s)                                           # on edges
    parts.append(0.5 * (V[fe[:, 1]] + V[fe[:, 2]]))                                                 # edge midpoints
    cen = V[fe].mean(1)
    nrm = np.cross(V[fe[:, 1]] - V[fe[:, 0]], V[fe[:, 2]] - V[fe[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    parts += [cen + 1e-3 * scale * nrm, cen - 1e-3 * scale * nrm]                                  # face centroids +- along the normal
    d = rng.normal(size=(200 if name == "ico7" else 500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    parts.append(0.5 * (lo + hi) + d * scale * rng.uniform(2, 5, size=(len(d), 1)))                # far outside
    if name == "torus":                                                                              # in the hole (off the axis)
        parts.append(np.stack([rng.uniform(-0.5, 0.5, 1000), rng.uniform(-0.5, 0.5, 1000), rng.uniform(-0.3, 0.3, 1000)], 1))
    n_box = max(2000, n_min - sum(len(p) for p in parts))
    parts.append(rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n_box, 3)))         # around and inside
    return np.ascontiguousarray(np.concatenate(parts)), scale


def _closest_on_tris(P, A, B, C):
    """closest points of triangles (A, B, C)[k] to points P[k], vectorised: the projection onto the plane when it falls inside,
    else the best of the three edge segments (not the region walk of the library's routine)"""
    n = np.cross(B - A, C - A)
    nn = np.einsum("ij,ij->i", n, n)
    t = np.einsum("ij,ij->i", P - A, n) / nn
    X = P - t[:, None] * n
    def side(U, W):
        return np.einsum("ij,ij->i", np.cross(W - U, X - U), n)
    inside = (side(A, B) >= 0) & (side(B, C) >= 0) & (side(C, A) >= 0)
    best = X.copy()
    bd = np.full(len(P), np.inf)
    for U, W in ((A, B), (B, C), (C, A)):
        e = W - U
        s = np.clip(np.einsum("ij,ij->i", P - U, e) / np.einsum("ij,ij->i", e, e), 0.0, 1.0)
        Q = U + s[:, None] * e
        dq = np.einsum("ij,ij->i", P - Q, P - Q)
        take = ~inside & (dq < bd)
        best[take] = Q[take]; bd = np.where(take, dq, bd)
    return best


def brute_force(V, F, P):
    """closest point of the mesh to every point by exhaustive search over the triangles that can hold it (a kd-tree over the triangle
    centroids only prunes triangles farther than the nearest vertex), ties to the lowest triangle index -> (proj, d2, tri)"""
    from scipy.spatial import cKDTree
    cen = V[F].mean(1)
    rad = np.linalg.norm(V[F] - cen[:, None, :], axis=2).max()
    dv, _ = cKDTree(V).query(P)
    cand = cKDTree(cen).query_ball_point(P, dv + rad + 1e-9)
    proj = np.empty_like(P); d2o = np.empty(len(P)); tri = np.empty(len(P), np.int64)
    chunk_p, chunk_t = [], []
    def flush():
        if not chunk_p:
            return
        pi = np.concatenate(chunk_p); ti = np.concatenate(chunk_t)
        Q = _closest_on_tris(P[pi], V[F[ti, 0]], V[F[ti, 1]], V[F[ti, 2]])
        d2 = np.einsum("ij,ij->i", P[pi] - Q, P[pi] - Q)
        o = np.lexsort((ti, d2, pi))
        first = np.ones(len(o), bool); first[1:] = pi[o][1:] != pi[o][:-1]
        sel = o[first]
        proj[pi[sel]] = Q[sel]; d2o[pi[sel]] = d2[sel]; tri[pi[sel]] = ti[sel]
        chunk_p.clear(); chunk_t.clear()
    tot = 0
    for i, c in enumerate(cand):
        chunk_p.append(np.full(len(c), i)); chunk_t.append(np.asarray(c, np.int64)); tot += len(c)
        if tot > 2_000_000:
            flush(); tot = 0
    flush()
    return proj, d2o, tri


def winding_inside(V, F, P, chunk=2048):
    """generalised winding number (van Oosterom & Strackee solid angles) > 1/2"""
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


def numpy_inside(name, V, F, P, tri):
    if name in ("cube", "torus", "ico2"):
        return winding_inside(V, F, P)
    # the icospheres are convex with small dihedral angles: inside iff below the plane of the nearest face
    n = np.cross(V[F[tri, 1]] - V[F[tri, 0]], V[F[tri, 2]] - V[F[tri, 0]])
    return np.einsum("ij,ij->i", P - V[F[tri, 0]], n) < 0


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _expect_error(pkg, V, F, *words):
    with pytest.raises(pkg.AdmmHipError) as e:
        pkg.Mesh(V, F)
    msg = str(e.value)
    for w in words:
        assert w in msg, msg
    return msg


def test_mesh_validation(pkg):
    V, F = cube()
    pkg.Mesh(V, F)                                                             # the valid cube is accepted
    _expect_error(pkg, V, F[1:], "open", "shared by 1 triangle")               # a triangle missing
    fin = np.array([[F[0, 0], F[0, 1], 8], [F[0, 1], F[0, 0], 8]], np.int32)   # a fin on a cube edge: 4 triangles at one edge
    Vf = np.concatenate([V, [[0.5, -0.5, 0.5]]])
    _expect_error(pkg, Vf, np.concatenate([F, fin]), "not edge-manifold", "shared by 4 triangles", "edge (%d, %d)" % tuple(sorted(F[0, :2])))
    Fl = F.copy(); Fl[5] = Fl[5, [0, 2, 1]]                                    # one triangle flipped
    _expect_error(pkg, V, Fl, "same direction", "triangle")
    Vd = V.copy(); Vd[F[3, 2]] = 0.5 * (V[F[3, 0]] + V[F[3, 1]])                 # triangle 3 collinear
    _expect_error(pkg, Vd, F, "triangle 3", "degenerate")
    Fr = F.copy(); Fr[4, 1] = 12
    _expect_error(pkg, V, Fr, "triangle 4", "out of range")
    Fi = F[:, [0, 2, 1]]                                                       # all inward
    _expect_error(pkg, V, Fi, "volume")


def test_registration_errors(pkg):
    V, F = cube()
    s = pkg.System(device_id=-1)
    x = np.random.default_rng(0).uniform(-1, 2, size=(40, 3))
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(40, dtype=np.int32), [32.0])
    mid = s.add_collision_mesh(V, F)
    assert mid == 0
    with pytest.raises(pkg.AdmmHipError) as e:
        s.set_collision_shapes([MESH], [[0, 0, 0, 1]])
    assert "mesh_id 1" in str(e.value) and "not a registered mesh" in str(e.value)
    s.set_collision_shapes([FLOOR, MESH], [[0, -1, 0, 0], [0, 0, 0, mid]])
    s.initialize()
    with pytest.raises(pkg.AdmmHipError) as e:
        s.add_collision_mesh(V, F)
    assert "error 3" in str(e.value) and "before finalize" in str(e.value)      # ADMM_ERR_STATE


@pytest.mark.parametrize("name", list(MESHES))
def test_query_vs_numpy_brute_force(pkg, name):
    V, F = mesh(name)
    P, scale = sample_points(name)
    assert len(P) >= 10000
    t = np.array([0.25, -0.5, 1.0])
    proj, sd = pkg.mesh_query(V, F, P + t, t)
    pnp, d2, tri = brute_force(V, F, P)
    err = np.abs(proj - t - pnp).max()
    assert err <= 1e-12 * scale, (name, err)
    assert np.allclose(np.abs(sd), np.sqrt(d2), rtol=0, atol=1e-12 * scale)
    far = np.sqrt(d2) > 1e-12
    ins = numpy_inside(name, V, F, P, tri)
    bad = np.nonzero(far & ((sd > 0) != ins))[0]
    assert bad.size == 0, (name, bad[:10], P[bad[:3]])
    assert 0 < ins[far].sum() < far.sum()                                         # both sides are sampled
    if name == "torus":                                                            # the hole is outside
        hole = np.linalg.norm(P[:, :2], axis=1) < 0.5
        assert hole.sum() > 500 and not (sd[hole] > 0).any()


@pytest.mark.parametrize("name", ["cube", "torus", "ico5"])
def test_query_deterministic_under_rotated_triangles(pkg, name):
    V, F = mesh(name)
    P, _ = sample_points(name, seed=1)
    a = pkg.mesh_query(V, F, P)
    b = pkg.mesh_query(V, F, P)
    rng = np.random.default_rng(5)
    sh = rng.integers(0, 3, size=len(F))
    Fr = np.stack([F[np.arange(len(F)), (sh + k) % 3] for k in range(3)], 1).astype(np.int32)
    assert not np.array_equal(Fr, F)
    c = pkg.mesh_query(V, Fr, P)
    for u, v in ((a, b), (a, c)):
        assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])


def test_bvh_depth_bounded(pkg):
    V, F = mesh("ico7")
    inf = pkg.Mesh(V, F).info()
    assert inf["n_tris"] == 327680 and inf["depth"] <= 32
    assert inf["n_nodes"] == 2 * (inf["n_nodes"] // 2) + 1                         # a full binary tree


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _points_system(pkg, P, types, params, meshes):
    s = pkg.System(device_id=0)
    s.set_timestep(0.02)
    n = len(P)
    s.add_nodes(P.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [32.0])
    for V, F in meshes:
        s.add_collision_mesh(V, F)
    s.set_collision_shapes(types, params)
    s.initialize()
    return s, b


def _device_project(s, b, P):
    n = len(P)
    s.write_local(b, u=np.zeros((n, 3)))
    s.local_step_dx(b, P)
    return s.read_local(b)["z"]


def _np_floor(p, cy):
    p = p.copy()
    hit = cy - p[:, 1] > 0
    p[hit, 1] = cy
    return p


def _np_sphere(p, c, R):
    d = p - c
    nrm = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    hit = R - nrm > 0
    q = p.copy()
    for j in range(3):
        q[hit, j] = c[j] + R * (d[hit, j] / nrm[hit])
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "torus", "ico2", "ico5", "ico7"])
def test_device_query_equals_host_query(pkg, name):
    V, F = mesh(name)
    P, scale = sample_points(name)
    t = np.array([0.1, 0.2, -0.3])
    P = np.ascontiguousarray(P + t)
    s, b = _points_system(pkg, P, [MESH], [[*t, 0]], [(V, F)])
    z = _device_project(s, b, P)
    proj, sd = pkg.mesh_query(V, F, P, t)
    want = np.where((sd > 0)[:, None], proj, P)
    assert (sd > 0).sum() > 1000
    assert np.array_equal(z, want), (name, np.abs(z - want).max(), np.count_nonzero((z != want).any(1)))
    # [floor, mesh, sphere] in one list: the analytic shapes through the same kernel, composed in list order
    cy, c, R = float(t[1] - 0.2), np.array([0.3, 0.0, 0.1]) + t, 0.45
    s2, b2 = _points_system(pkg, P, [FLOOR, MESH, SPHERE], [[0, cy, 0, 0], [*t, 0], [*c, R]], [(V, F)])
    z2 = _device_project(s2, b2, P)
    p = _np_floor(P, cy)
    proj, sd = pkg.mesh_query(V, F, p, t)
    p = np.where((sd > 0)[:, None], proj, p)
    p = _np_sphere(p, c, R)
    assert np.array_equal(z2, p), (name, np.abs(z2 - p).max())


def _bar_scene(pkg, mesh_specs, shapes_fn, nx=6, ny=4, nz=24, rank=0, world=1, mode=None):
    """a linear-tet cantilever (anchored at z = 0) falling under gravity, a collision force over all its nodes.
    mesh_specs: meshes to register; shapes_fn(frame) -> (types, params) of that frame's list"""
    mg = pkg.meshgen
    x, tets = mg.bar(nx, ny, nz)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    s = pkg.System(device_id=0)
    s.set_timestep(0.02)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["ANCHOR"], mg.bar_anchor_nodes(nx, ny), [-1.0, 1.0])
    b = s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity([0.0, -9.8, 0.0])
    for V, F in mesh_specs:
        s.add_collision_mesh(V, F)
    s.set_collision_shapes(*shapes_fn(0))
    if world > 1:
        s.set_shard(rank, world)
        if mode:
            s.set_shard_mode(mode)
    s.coll_batch = b
    s.n_x = len(x)
    return s


def _obstacle(frame, nx=6, ny=4, nz=24, h=0.05):
    """an icosphere of radius 0.3 under the bar's free end, rising by 2 mm a frame"""
    return np.array([nx * h / 2, -0.34 + 0.002 * frame, nz * h * 0.8])


def _run(s, frames, iters=10):
    out = []
    for f in range(frames):
        s.step(iters)
        out.append(s.m_x.copy())
    return out


@pytest.mark.gpu
def test_unreachable_mesh_leaves_frames_bitwise_equal(pkg):
    """a mesh registered and listed, but placed where no node reaches its box: every frame as without any mesh (floor + sphere)"""
    V, F = mesh("ico5")
    an = lambda f: ([FLOOR, SPHERE], [[0, -0.3, 0, 0], [0.15, -0.25, 1.0, 0.2]])
    withm = lambda f: ([FLOOR, MESH, SPHERE], [[0, -0.3, 0, 0], [100.0, 100.0, 100.0, 0], [0.15, -0.25, 1.0, 0.2]])
    a = _bar_scene(pkg, [], an); a.initialize()
    b = _bar_scene(pkg, [(V, F)], withm); b.initialize()
    xa, xb = _run(a, 12), _run(b, 12)
    for f in range(12):
        assert np.array_equal(xa[f], xb[f]), f
    assert xa[-1].reshape(-1, 3)[:, 1].min() < -0.2                             # the bar did reach the analytic shapes


def _mesh_scene_frames(pkg, frames=10, **kw):
    V, F = mesh("ico5")
    V = V * 0.3
    sh = lambda f: ([FLOOR, MESH], [[0, -0.6, 0, 0], [*_obstacle(f), 0]])
    s = _bar_scene(pkg, [(V, F)], sh, **kw)
    return s, sh


@pytest.mark.gpu
def test_mesh_scene_contact_and_launch_modes(pkg, monkeypatch):
    """the mesh scene (a moving icosphere obstacle) under every launch mode: bitwise the same frames; the obstacle is really hit"""
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {"ADMM_HIP_LOCAL_MULTI": "0"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s, sh = _mesh_scene_frames(pkg)
        s.initialize()
        xs, near = [], 0
        for f in range(10):
            s.set_collision_shapes(*sh(f))
            s.step(10)
            xs.append(s.m_x.copy())
            near = max(near, int((np.linalg.norm(xs[-1].reshape(-1, 3) - _obstacle(f), axis=1) < 0.31).sum()))
        res[tuple(env.items())] = (xs, near, s.graph_state())
    keys = list(res)
    for k in keys[1:]:
        for f in range(10):
            assert np.array_equal(res[keys[0]][0][f], res[k][0][f]), (k, f)
    g = res[keys[0]][2]
    assert g["iter_graph"] or g["frame_graph_iters"] > 0                             # GRAPH=1 did replay graphs
    # contact: nodes rest on the obstacle's surface (radius 0.3) and none went deep into it
    x = res[keys[0]][0][-1].reshape(-1, 3)
    r = np.linalg.norm(x - _obstacle(9), axis=1)
    print("mesh scene: %d of %d nodes within 1 cm of the obstacle at most, closest %.4f" % (res[keys[0]][1], len(x), r.min()))
    assert res[keys[0]][1] > 0 and r.min() > 0.25


@pytest.mark.gpu
def test_mesh_scene_two_subtree_shards(pkg, monkeypatch):
    """the mesh scene as two subtree shards on one GPU: each rank registers the same mesh; the ranks end bitwise identical and match
    the unsharded run (linear tets: no truncated minimiser, so only the order of the partial sums differs)"""
    from test_sharding import _run_sharded, _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    ref, _ = _mesh_scene_frames(pkg)
    ref.initialize()
    shards = [_mesh_scene_frames(pkg, rank=r, world=2, mode="subtree")[0] for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    assert sum(s.info()["n_elems_local"] for s in shards) == ref.info()["n_elems_total"]
    b = np.random.default_rng(2).normal(size=3 * ref.n_nodes)
    xref = ref.solve_only(b)
    out = _run_sharded(shards, 6, 10, b)
    refx = _run(ref, 6)
    for r in range(2):
        sol, xs, vs = out[r]
        assert np.abs(sol - xref).max() < 1e-10 * np.abs(xref).max()
        for f in range(6):
            assert np.abs(xs[f] - refx[f]).max() < 1e-9, (r, f, np.abs(xs[f] - refx[f]).max())
        assert np.array_equal(xs[-1], out[0][1][-1]) and np.array_equal(vs, out[0][2])
    r = np.linalg.norm(refx[-1].reshape(-1, 3) - _obstacle(0), axis=1)
    assert (r < 0.31).any()                                                        # contact happened


# ---------------------------------------------------------------------------------------------------------------------------------
# the class API end to end: CollisionMesh (device) against HostMesh (a subclass: host-projected through the generic batch)
# ---------------------------------------------------------------------------------------------------------------------------------
def _scene_mesh_input(pkg, path):
    V, F = mesh("ico5")
    V = V * 0.6
    x, tets = pkg.meshgen.bar(16, 3, 16)
    m = pkg.meshgen.lumped_tet_mass(x, tets, 1000.0)
    x = x + np.array([0.0, 0.02, 0.0])
    c0 = np.array([0.4, -0.6, 0.4, 0.001])            # centre (the plate's middle, top of the sphere at y = 0), rise per frame
    with open(path, "wb") as f:
        np.array([len(V), len(F), len(x), len(tets)], np.int32).tofile(f)
        V.astype(np.float64).tofile(f); F.astype(np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f); tets.astype(np.int32).tofile(f); c0.tofile(f)
    return V, F, x, c0


@pytest.mark.gpu
def test_class_api_mesh_vs_host_projected(pkg, tmp_path):
    import subprocess
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_mesh", pkg)
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
        print("class API: the control (user floor vs built-in floor) is bitwise equal, so the mesh pair must be too: max diff %g" % diff)
        assert diff == 0.0
    else:
        print("class API: the control differs by %g, the mesh pair by %g" % (control, diff))
        assert diff <= control
    touched = np.zeros(n, bool)
    for f in range(frames):
        t = c0[:3] + np.array([0.0, c0[3] * f, 0.0])
        _, sd = pkg.mesh_query(V, F, out[2][f], t)
        touched |= sd > -5e-3
    print("class API: %d of %d nodes (%.1f %%) reached the obstacle" % (touched.sum(), n, 100.0 * touched.mean()))
    assert touched.mean() >= 0.05
