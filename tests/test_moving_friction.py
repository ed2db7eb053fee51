"""Contact friction against obstacles that move and against body surfaces (admm_hip_set_collision_motion, admm_hip_set_collision_mesh_velocity,
admm_hip_set_body_surface_friction): the rule's moving form and the vertex-velocity interpolation on the host against numpy, the argument
checks, closed forms of a particle on a conveyor, and on the GPU: the moving form of the friction kernel bit for bit against the host
routines (rigid motions, meshes with vertex velocities, a body surface), zero motion as the existing path, whole frames against the numpy
particle recursion, a slab carried by a moving platform, two stacked slabs, launch modes, subtree shards, residual tracking, the class API.

No reference counterpart: the expected values come from numpy in here."""

import subprocess

import numpy as np
import pytest

from checkers import KIND
from test_collision_friction import (CYLINDER, DT, G, SLAB, W, _bar, _bar_frames, _expect, _kernel_case, _np_cylinder, _np_friction, _particle_scene,
                                     _points_system, _same, _tilt)
from test_collision_mesh import FLOOR, MESH, SPHERE, _np_floor, _np_sphere, mesh

EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule's moving form, the rigid displacement and the particle recursion in numpy
# ---------------------------------------------------------------------------------------------------------------------------------
def _np_friction_moving(p, po, x0, w, mu):
    """the rule of include/admm_hip.h with r = (p' - x0) - w, row by row; the dtype of p decides the precision -> (result, mode, tl, lim)"""
    p, po, x0, w = np.asarray(p), np.asarray(po), np.asarray(x0), np.asarray(w)
    mu = np.broadcast_to(np.asarray(mu, dtype=p.dtype), (len(p),))
    d = po - p
    depth = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    on = (mu > 0) & (depth > 0)
    n = d / np.where(on, depth, 1)[:, None]
    r = (po - x0) - w
    rn = r[:, 0] * n[:, 0] + (r[:, 1] * n[:, 1] + r[:, 2] * n[:, 2])
    t = r - rn[:, None] * n
    tl = np.sqrt(t[:, 0] * t[:, 0] + (t[:, 1] * t[:, 1] + t[:, 2] * t[:, 2]))
    with np.errstate(invalid="ignore"):
        lim = np.where(on, mu * depth, 0)
    stick = on & (tl <= lim)
    slip = on & ~stick
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(slip, lim / np.where(slip, tl, 1), 0)
    out = np.where(stick[:, None], po - t, np.where(slip[:, None], po - s[:, None] * t, po))
    return out, np.where(stick, 1, np.where(slip, 2, 0)).astype(np.int32), tl, lim


def _np_rigid(m, c, dt=DT):
    """w_rigid at the points c [n][3] for the motion m[9] = (a, om, o), in the order include/admm_hip.h documents"""
    m = np.asarray(m, dtype=np.float64)
    e0, e1, e2 = c[:, 0] - m[6], c[:, 1] - m[7], c[:, 2] - m[8]
    x0 = m[4] * e2 - m[5] * e1
    x1 = m[5] * e0 - m[3] * e2
    x2 = m[3] * e1 - m[4] * e0
    return np.stack([dt * (m[0] + x0), dt * (m[1] + x1), dt * (m[2] + x2)], 1)


def _belt_particles(x, v, g, mu, vb, frames, iters, m=1.0):
    """test_collision_friction._particles on a floor y = 0 that moves tangentially at vb: the ADMM recursion of admm_hip_step with the
    rule's moving form, w = DT vb -> (x, v per frame, the mode of the last projection: -1 airborne)"""
    x, v = x.copy(), v.copy()
    u = np.zeros_like(x)
    k = DT * DT * W * W
    w = np.broadcast_to(DT * (np.asarray(vb, dtype=np.float64) + 0.0), x.shape)
    xs, vs, last = [], [], None
    for _ in range(frames):
        v = v + DT * g
        xbar = x + DT * v
        xc = xbar.copy()
        for _ in range(iters):
            p = xc + u
            z = _np_floor(p, 0.0)
            hit = (z != p).any(1)
            z, mode, _, _ = _np_friction_moving(p, z, x, w, mu)
            last = np.where(hit, mode, -1)
            u = u + (xc - z)
            xc = (m * xbar + k * (z - u)) / (m + k)
        v = (xc - x) / DT
        x = xc
        xs.append(x.copy()); vs.append(v.copy())
    return xs, vs, last


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_friction_query_moving_vs_longdouble(pkg):
    """4096 random cases as in test_friction_query_vs_longdouble, with w in [-0.5, 0.5]^3: modes exact, the result within
    64 eps max(1, |p|, |x0|, |w|); w = 0 gives the bits of friction_query"""
    n = 4096
    rng = np.random.default_rng(12)
    mus = np.array([0.0, 0.1, 0.5, 2.0, np.inf])
    L = np.longdouble

    def draw(k):
        return rng.uniform(-2, 2, (k, 3)), rng.uniform(-2, 2, (k, 3)), rng.uniform(-2, 2, (k, 3)), rng.uniform(-0.5, 0.5, (k, 3)), mus[rng.integers(0, 5, k)]
    p, po, x0, w, mu = draw(n)
    redrawn = 0
    for _ in range(20):
        _, _, tl, lim = _np_friction_moving(p.astype(L), po.astype(L), x0.astype(L), w.astype(L), mu.astype(L))
        depth = np.linalg.norm(po - p, axis=1)
        bad = np.nonzero((np.abs(tl - lim) < 1e-6) | (depth < 1e-3))[0]
        if bad.size == 0:
            break
        redrawn += bad.size
        p[bad], po[bad], x0[bad], w[bad], mu[bad] = draw(bad.size)
    assert bad.size == 0 and redrawn <= n // 100, redrawn
    want, wmode, _, _ = _np_friction_moving(p.astype(L), po.astype(L), x0.astype(L), w.astype(L), mu.astype(L))
    got, mode = pkg.friction_query_moving(p, po, x0, w, mu)
    assert np.array_equal(mode, wmode)
    for k in range(3):
        assert (mode == k).sum() >= 10, (k, (mode == k).sum())
    nrm = lambda a: np.linalg.norm(a, axis=1)
    tol = 64 * EPS * np.maximum(1.0, np.maximum(np.maximum(nrm(p), nrm(x0)), nrm(w)))
    err = np.abs((got.astype(L) - want).astype(np.float64)).max(1)
    print("friction_query_moving vs longdouble: max error %.3g, smallest bound %.3g, worst ratio %.3g" % (err.max(), tol.min(), (err / tol).max()))
    assert (err <= tol).all(), (err / tol).max()
    # the float64 restatement in the same order: the same bits
    same, smode, _, _ = _np_friction_moving(p, po, x0, w, mu)
    assert np.array_equal(got, same) and np.array_equal(mode, smode)
    # w = 0: friction_query
    a, am = pkg.friction_query(p, po, x0, mu)
    b, bm = pkg.friction_query_moving(p, po, x0, np.zeros_like(p), mu)
    assert np.array_equal(a, b) and np.array_equal(am, bm)
    assert np.abs(a - got).max() > 1e-3                                            # and w matters


def _np_closest_weights(A, B, C, P):
    """independent barycentric coordinates of the closest point of triangle (A, B, C) to P by projected clamping (float64)"""
    out = np.zeros((len(P), 3))
    for i in range(len(P)):
        a, b, c, p = A[i], B[i], C[i], P[i]
        best = None
        # face
        n = np.cross(b - a, c - a)
        M = np.stack([b - a, c - a, n], 1)
        s = np.linalg.solve(M, p - a)
        cands = []
        if s[0] >= 0 and s[1] >= 0 and s[0] + s[1] <= 1:
            cands.append(np.array([1 - s[0] - s[1], s[0], s[1]]))
        for (i0, i1, q0, q1) in ((0, 1, a, b), (1, 2, b, c), (2, 0, c, a)):
            t = np.clip(np.dot(p - q0, q1 - q0) / np.dot(q1 - q0, q1 - q0), 0, 1)
            wv = np.zeros(3); wv[i0] = 1 - t; wv[i1] = t
            cands.append(wv)
        for wv in cands:
            d = np.linalg.norm(wv[0] * a + wv[1] * b + wv[2] * c - p)
            if best is None or d < best[0]:
                best = (d, wv)
        out[i] = best[1]
    return out


@pytest.mark.parametrize("name", ["cube", "ico2"])
def test_mesh_velocity_query(pkg, name):
    """weights >= 0 summing to 1 within 4 eps; sum b_i corner_i = mesh_query's closest point and a linear field A x + b is reproduced at
    it, both to 1e-12 scale; at least 5 hits in each of the face, edge and vertex regions"""
    V, F = mesh(name)
    rng = np.random.default_rng(7)
    t = np.array([0.1, -0.2, 0.3])
    lo, hi = V.min(0), V.max(0)
    ctr, ext = (lo + hi) / 2, (hi - lo).max()
    P = ctr + ext * rng.uniform(-1.2, 1.2, (600, 3)) + t
    # points right over vertices and edge midpoints, pushed outwards: vertex and edge regions
    out_dir = V - ctr
    out_dir /= np.linalg.norm(out_dir, axis=1)[:, None]
    pv = V[:40] + 0.3 * ext * out_dir[:40] + t
    P = np.concatenate([P, pv])
    A = rng.normal(size=(3, 3)); bvec = rng.normal(size=3)
    vel = V @ A.T + bvec
    out, wts, ids = pkg.mesh_velocity_query(V, F, P, vel, t)
    proj, _ = pkg.mesh_query(V, F, P, t)
    scale = max(1.0, np.abs(V).max(), np.abs(P).max())
    assert (wts >= 0).all() and np.abs(wts.sum(1) - 1).max() <= 4 * EPS, (wts.min(), np.abs(wts.sum(1) - 1).max())
    assert ((ids >= 0) & (ids < len(V))).all()
    rec = (wts[:, :, None] * V[ids]).sum(1) + t
    assert np.abs(rec - proj).max() <= 1e-12 * scale, np.abs(rec - proj).max()
    lin = (proj - t) @ A.T + bvec
    vscale = max(1.0, np.abs(vel).max())
    assert np.abs(out - lin).max() <= 1e-12 * scale * vscale, np.abs(out - lin).max()
    # the documented order, bitwise
    va, vb, vc = vel[ids[:, 0]], vel[ids[:, 1]], vel[ids[:, 2]]
    assert np.array_equal(out, wts[:, 0:1] * va + (wts[:, 1:2] * vb + wts[:, 2:3] * vc))
    # the corners are a triangle of the mesh
    tri_set = {tuple(sorted(f)) for f in F.tolist()}
    assert all(tuple(sorted(r)) in tri_set for r in ids.tolist())
    nz = (wts > 0).sum(1)
    counts = [int((nz == k).sum()) for k in (3, 2, 1)]
    print("%s: face / edge / vertex hits %s" % (name, counts))
    assert min(counts) >= 5, counts
    # against an independent closest point on the same triangle
    ref = _np_closest_weights(V[ids[:, 0]], V[ids[:, 1]], V[ids[:, 2]], P - t)
    assert np.abs(ref - wts).max() <= 1e-9, np.abs(ref - wts).max()


def test_moving_friction_argument_checks(pkg):
    """a host-only context: every refusal of the three setters, each naming its entry, mesh or vertex; the motions a new list keeps (the
    same length) or loses (another length), seen through which lists finalize and set_collision_shapes then accept"""
    mg = pkg.meshgen
    xb, tets = mg.bar(1, 1, 1)
    x = np.concatenate([xb, np.random.default_rng(0).uniform(-1, 2, size=(40, 3))])
    Vc, Fc = mesh("cube")
    s = pkg.System(device_id=-1)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    sid = s.add_body_surface(0, len(xb), mg.tet_surface(tets))
    cid = s.add_collision_mesh(Vc, Fc)
    floor, sph, body, cub = [0, -1, 0, 0], [0.5, 0.5, 0.5, 0.2], [0, 0, 0, sid], [3, 3, 3, cid]
    s.set_collision_shapes([FLOOR, SPHERE, MESH], [floor, sph, body])
    z9 = [0.0] * 9
    mv = [1.0, 0, 0, 0, 0, 2.0, 0.5, 0.5, 0.5]
    _expect(pkg, lambda: s.set_collision_motion([mv, z9]), "error 1", "2 motions", "3 entries")
    _expect(pkg, lambda: s.set_collision_motion([mv, [0, 0, np.inf, 0, 0, 0, 0, 0, 0], z9]), "error 1", "shape 1", "not finite")
    _expect(pkg, lambda: s.set_collision_motion([z9, z9, [0, 0, 0, 0, np.nan, 0, 0, 0, 0]]), "error 1", "shape 2")
    _expect(pkg, lambda: s.set_collision_motion([mv, z9, mv]), "error 1", "shape 2", "body surface")
    _expect(pkg, lambda: s.set_collision_mesh_velocity(cid, np.zeros((8, 3))), "error 3", "after finalize")
    _expect(pkg, lambda: s.set_body_surface_friction(cid, 0.5), "error 1", "mesh_id %d" % cid, "not a body surface")
    _expect(pkg, lambda: s.set_body_surface_friction(7, 0.5), "error 1", "mesh_id 7")
    _expect(pkg, lambda: s.set_body_surface_friction(sid, -0.5), "error 1", "body surface %d" % sid, "negative")
    _expect(pkg, lambda: s.set_body_surface_friction(sid, np.nan), "error 1", "body surface %d" % sid)
    s.set_body_surface_friction(sid, np.inf)                                       # +inf is a coefficient; before finalize
    s.set_collision_motion([mv, mv, z9])
    # the same length keeps the motions: the body surface moves to entry 1, where one is set -> refused, naming it
    _expect(pkg, lambda: s.set_collision_shapes([FLOOR, MESH, SPHERE], [floor, body, sph]), "error 1", "shape 1", "body surface", "rigid motion")
    # another length zeroes them: back at three entries the same list is accepted, and by finalize too
    s.set_collision_shapes([FLOOR, MESH], [floor, body])
    s.set_collision_shapes([FLOOR, MESH, SPHERE], [floor, body, sph])
    s.initialize()
    # after finalize
    _expect(pkg, lambda: s.set_collision_motion([z9, mv, z9]), "shape 1", "body surface")
    _expect(pkg, lambda: s.set_collision_motion([z9]), "1 motions", "3 entries")
    s.set_collision_motion([mv, z9, mv])
    _expect(pkg, lambda: s.set_collision_shapes([MESH, FLOOR, SPHERE], [body, floor, sph]), "shape 0", "body surface")
    s.set_collision_shapes([SPHERE, MESH, FLOOR], [sph, body, floor])              # (mv, 0, mv) kept: the body's entry has 0
    s.set_collision_shapes([FLOOR], [floor])
    s.set_collision_shapes([MESH, FLOOR, MESH], [body, floor, cub])                # zeroed by the change of length: accepted now
    s.set_body_surface_friction(sid, 0.25)
    _expect(pkg, lambda: s.set_collision_mesh_velocity(sid, np.zeros((8, 3))), "error 1", "mesh %d" % sid, "body surface")
    _expect(pkg, lambda: s.set_collision_mesh_velocity(9, np.zeros((8, 3))), "error 1", "mesh_id 9")
    _expect(pkg, lambda: s.set_collision_mesh_velocity(cid, np.zeros((7, 3))), "error 1", "mesh %d" % cid, "7 vertex velocities", "8 vertices")
    bad = np.zeros((8, 3)); bad[5, 1] = np.inf
    _expect(pkg, lambda: s.set_collision_mesh_velocity(cid, bad), "error 1", "mesh %d" % cid, "vertex 5", "not finite")
    s.set_collision_mesh_velocity(cid, np.ones((8, 3)))
    s.set_collision_mesh_velocity(cid, None)


def test_belt_particle_closed_forms():
    """the numpy recursion the GPU test compares with, at 100 iterations a frame, on a level floor moving at vb = (1, 0, 0): with
    mu = inf a particle released at rest moves vb dt per frame after the first contact frame; with mu = 0.5 it gains mu g dt = 0.098 a
    frame until it has the belt's speed, and in the belt's frame it has then travelled the stopping distance of
    test_particle_model_closed_forms, 0.0922"""
    z3 = np.zeros((1, 3))
    g = np.array([0.0, -G, 0.0])
    vb = np.array([1.0, 0.0, 0.0])
    xs, vs, last = _belt_particles(z3, z3, g, np.inf, vb, 12, 100)
    adv = np.diff(np.array(xs)[:, 0, :], axis=0)
    assert last[0] == 1 and np.abs(adv - DT * vb).max() <= 1e-12, np.abs(adv - DT * vb).max()
    xs, vs, _ = _belt_particles(z3, z3, g, 0.5, vb, 40, 100)
    for k in range(1, 11):
        assert abs(vs[k - 1][0, 0] - 0.098 * k) <= 1e-6, (k, vs[k - 1][0, 0])
    assert np.abs(vs[-1][0] - vb).max() <= 1e-9
    assert abs((40 * DT * vb[0] - xs[-1][0, 0]) - 0.0922) <= 1e-6, 40 * DT * vb[0] - xs[-1][0, 0]
    # a belt at rest is test_collision_friction's model
    from test_collision_friction import _particles
    v1 = np.array([[1.0, 0, 0]])
    a = _belt_particles(z3, v1, g, 0.5, np.zeros(3), 10, 20)
    b = _particles(z3, v1, g, lambda f: 0.5, 10, 20)
    assert all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the host routines
# ---------------------------------------------------------------------------------------------------------------------------------
def _compose_moving(pkg, p, x0, steps):
    """the list's pushes in order, the moving rule after each; a step = (push(p) -> (q, w_extra or None), mu, motion[9]) ->
    (z, modes of the applications that moved a point)"""
    modes = []
    for push, mu, motion in steps:
        q, extra = push(p)
        moved = (q != p).any(1)
        w = _np_rigid(motion, q)
        if extra is not None:
            w = w + extra
        q, mode = pkg.friction_query_moving(p, q, x0, w, mu)
        modes.append(mode[moved])
        p = q
    return p, np.concatenate(modes)


Z9 = [0.0] * 9
RIGID_MU = [0.3, 0.0, 0.7, np.inf]
RIGID_MOTION = [[0.9, 0.0, -0.6, 0, 0, 0, 0, 0, 0], Z9, [0, 0, 0, 1.5, -2.0, 2.5, -0.2, 0.1, 0.6], [0.5, -0.4, 0.7, 0, 0, 3.0, 0.3, 0.9, 0.0]]
RIGID_GEO = dict(cy=-0.4, c1=np.array([0.5, 0.2, 0.0]), R1=0.6, c2=np.array([-0.5, 0.3, 0.2]), R2=0.6, cc=np.array([0.0, 0.6, 0.0]), Rc=0.4)


def _rigid_system(pkg, x0, mu=RIGID_MU):
    g = RIGID_GEO
    return _points_system(pkg, x0, [FLOOR, SPHERE, SPHERE, CYLINDER], [[0, g["cy"], 0, 0], [*g["c1"], g["R1"]], [*g["c2"], g["R2"]], [*g["cc"], g["Rc"]]], mu)


def _rigid_want(pkg, dx, x0, u, motion=RIGID_MOTION):
    g = RIGID_GEO
    plain = lambda f: (lambda p: (f(p), None))
    return _compose_moving(pkg, dx + u, x0, [(plain(lambda p: _np_floor(p, g["cy"])), RIGID_MU[0], motion[0]),
                                             (plain(lambda p: _np_sphere(p, g["c1"], g["R1"])), RIGID_MU[1], motion[1]),
                                             (plain(lambda p: _np_sphere(p, g["c2"], g["R2"])), RIGID_MU[2], motion[2]),
                                             (plain(lambda p: _np_cylinder(p, g["cc"], g["Rc"])), RIGID_MU[3], motion[3])])


def test_rigid_case_counts(pkg):
    """the seeds of the GPU kernel tests, checked on the host: at least 10 none, stick and slip (rigid), 10 stick and slip at mesh hits"""
    dx, x0, u = _kernel_case(200, 3)
    _, modes = _rigid_want(pkg, dx, x0, u)
    counts = [int((modes == k).sum()) for k in range(3)]
    assert min(counts) >= 10, counts
    _, modes, mesh_modes = _mesh_want(pkg, *_kernel_case(200, 4))
    assert (mesh_modes == 1).sum() >= 10 and (mesh_modes == 2).sum() >= 10, [int((mesh_modes == k).sum()) for k in range(3)]


@pytest.mark.gpu
def test_kernel_equals_host_rigid(pkg):
    """200 nodes, [floor 0.3, sphere 0, sphere 0.7, z-cylinder inf]; the floor translates, the second sphere rotates about an off-centre
    pivot, the cylinder does both: z and u bitwise against numpy pushes, numpy w_rigid in the documented order and friction_query_moving"""
    dx, x0, u = _kernel_case(200, 3)
    s, b = _rigid_system(pkg, x0)
    s.set_collision_motion(RIGID_MOTION)
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    want, modes = _rigid_want(pkg, dx, x0, u)
    counts = [int((modes == k).sum()) for k in range(3)]
    print("rigid motions: none / stick / slip among the pushes:", counts)
    assert min(counts) >= 10, counts
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.count_nonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))
    still, _ = _rigid_want(pkg, dx, x0, u, [Z9] * 4)
    assert np.abs(still - want).max() > 1e-3                                       # the motion matters


MESH_GEO = dict(tc=np.array([-0.6, -0.3, -0.5]), ti=np.array([0.4, 0.3, 0.2]), cy=-0.5)
MESH_MU = [0.2, 0.5, 0.5]
ICO_MOTION = [0.4, 0.2, -0.3, 1.0, 2.0, -1.5, 0.5, 0.2, 0.1]


def _mesh_fields():
    Vc, Fc = mesh("cube")
    Vi, Fi = mesh("ico2")
    Vi = Vi * 0.7
    velc = np.stack([0.8 * np.sin(3 * Vc[:, 1]) + 0.5 * Vc[:, 2] ** 2, -0.6 * Vc[:, 0] * Vc[:, 2], 0.7 * np.cos(2 * Vc[:, 0]) - 0.4], 1)      # not rigid
    veli = np.stack([0.5 * Vi[:, 0] ** 2, 0.6 * np.sin(4 * Vi[:, 2]), -0.5 * Vi[:, 0] * Vi[:, 1]], 1)
    return (Vc, Fc, velc), (Vi, Fi, veli)


def _mesh_want(pkg, dx, x0, u, moving=True):
    (Vc, Fc, velc), (Vi, Fi, veli) = _mesh_fields()
    g = MESH_GEO
    own = np.arange(len(dx)) < 60
    mesh_modes = []

    def mesh_push(V, F, vel, t, skip=None):
        def push(p):
            proj, sd = pkg.mesh_query(V, F, p, t)
            hit = sd > 0
            if skip is not None:
                hit &= ~skip
            vi, _, _ = pkg.mesh_velocity_query(V, F, p, vel, t)
            return np.where(hit[:, None], proj, p), (DT * vi if moving else None)
        return push
    want, modes = _compose_moving(pkg, dx + u, x0, [(lambda p: (_np_floor(p, g["cy"]), None), MESH_MU[0], Z9),
                                                    (mesh_push(Vc, Fc, velc, g["tc"], own), MESH_MU[1], Z9),
                                                    (mesh_push(Vi, Fi, veli, g["ti"]), MESH_MU[2], ICO_MOTION if moving else Z9)])
    # the modes at mesh hits alone
    p = _np_floor(dx + u, g["cy"])
    p, _ = pkg.friction_query_moving(dx + u, p, x0, np.zeros_like(p), MESH_MU[0])
    for push, mu, mo in ((mesh_push(Vc, Fc, velc, g["tc"], own), MESH_MU[1], Z9), (mesh_push(Vi, Fi, veli, g["ti"]), MESH_MU[2], ICO_MOTION if moving else Z9)):
        q, extra = push(p)
        moved = (q != p).any(1)
        w = _np_rigid(mo, q) + (extra if extra is not None else 0.0)
        q, mode = pkg.friction_query_moving(p, q, x0, w, mu)
        mesh_modes.append(mode[moved])
        p = q
    assert np.array_equal(p, want)
    return want, modes, np.concatenate(mesh_modes)


def _mesh_system(pkg, x0):
    (Vc, Fc, _), (Vi, Fi, _) = _mesh_fields()
    g = MESH_GEO
    return _points_system(pkg, x0, [FLOOR, MESH, MESH], [[0, g["cy"], 0, 0], [*g["tc"], 0], [*g["ti"], 1]], MESH_MU, meshes=[(Vc, Fc), (Vi, Fi)], owner=(0, 0, 60))


@pytest.mark.gpu
def test_kernel_equals_host_meshes(pkg):
    """[floor 0.2, cube 0.5, ico2 0.5], the cube owned by the first 60 nodes; the cube has per-vertex velocities from a field that is not
    rigid, the ico2 a rigid motion and per-vertex velocities together: z and u bitwise through mesh_query, mesh_velocity_query and
    friction_query_moving; owners inside the cube are untouched"""
    (Vc, Fc, velc), (Vi, Fi, veli) = _mesh_fields()
    dx, x0, u = _kernel_case(200, 4)
    s, b = _mesh_system(pkg, x0)
    s.set_collision_mesh_velocity(0, velc)
    s.set_collision_mesh_velocity(1, veli)
    s.set_collision_motion([Z9, Z9, ICO_MOTION])
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    want, modes, mesh_modes = _mesh_want(pkg, dx, x0, u)
    counts = [int((mesh_modes == k).sum()) for k in range(3)]
    print("moving meshes: none / stick / slip at mesh hits:", counts)
    assert counts[1] >= 10 and counts[2] >= 10, counts
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.count_nonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))
    still, _, _ = _mesh_want(pkg, dx, x0, u, moving=False)
    assert np.abs(still - want).max() > 1e-3
    g = MESH_GEO
    p = dx + u
    own = np.arange(200) < 60
    _, sd = pkg.mesh_query(Vc, Fc, p, g["tc"])
    _, sdi = pkg.mesh_query(Vi, Fi, p, g["ti"])
    free = own & (sd > 0) & (p[:, 1] >= g["cy"]) & (sdi <= 0)
    assert free.sum() >= 3, free.sum()
    assert np.array_equal(r["z"][free], p[free])
    # velocities cleared again and the motion zeroed: the existing friction kernel's bits
    s.set_collision_mesh_velocity(0, None); s.set_collision_mesh_velocity(1, None)
    s.set_collision_motion([Z9] * 3)
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    assert np.array_equal(s.read_local(b)["z"], still)


@pytest.mark.gpu
def test_zero_motion_is_the_existing_path(pkg):
    """the two kernel scenes and the tet bar of test_collision_friction over 5 frames: with all motions zero the results are bitwise
    those of a context that never made the new calls, and a motion set and zeroed again between frames returns to those bits"""
    for case, make, seed in (("rigid", _rigid_system, 3), ("meshes", _mesh_system, 4)):
        dx, x0, u = _kernel_case(200, seed)
        n_sh = 4 if case == "rigid" else 3
        outs = []
        for variant in range(3):
            s, b = make(pkg, x0)
            if variant == 1:
                s.set_collision_motion([Z9] * n_sh)
            if variant == 2:
                s.set_collision_motion([[0.3] * 9] * n_sh)
                s.write_local(b, u=u); s.local_step_dx(b, dx)
                s.set_collision_motion([Z9] * n_sh)
            s.write_local(b, u=u)
            s.local_step_dx(b, dx)
            r = s.read_local(b)
            outs.append((r["z"].copy(), r["u"].copy()))
        for o in outs[1:]:
            assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]), case
    mu = [0.5, 0.25]
    a = _bar(pkg); a.set_collision_friction(mu); a.initialize()
    x_start = a.m_x.copy()
    fa = _bar_frames(a, 5)
    b = _bar(pkg); b.set_collision_friction(mu); b.set_collision_motion([Z9, Z9]); b.initialize()
    assert _same(fa, _bar_frames(b, 5))
    c = _bar(pkg); c.set_collision_friction(mu); c.initialize()
    c.set_collision_motion([[0.5, 0, 0.2, 0, 0, 0, 0, 0, 0], Z9])
    fc = _bar_frames(c, 5)                                                       # (the bar reaches the floor within five frames)
    assert c.graph_state()["graph_launches"] > 0 and _same(fa[:2], fc[:2]) and not _same(fa, fc)
    c.set_collision_motion([Z9, Z9])
    c.m_x = x_start; c.m_v = np.zeros_like(x_start)
    for bt in range(3):
        c.write_local(bt, u=np.zeros_like(fa[0][2][bt]))
    assert _same(fa, _bar_frames(c, 5))


def _body_case(pkg, seed=8, n=200):
    """a 2 x 2 x 2-cell tet body with a non-uniform velocity and 200 free nodes around and inside it"""
    mg = pkg.meshgen
    xb, tets = mg.bar(2, 2, 2)
    rng = np.random.default_rng(seed)
    nb = len(xb)
    xf = rng.uniform(-0.02, 0.12, (n, 3))
    u = np.where((rng.uniform(size=n) < 0.5)[:, None], 0.001, 0.02) * rng.normal(size=(n, 3))
    x = np.concatenate([xb, xf])
    v = np.zeros_like(x)
    v[:nb] = 0.4 * np.stack([0.6 * np.sin(20 * xb[:, 1]) + 0.3, -0.5 * np.cos(15 * xb[:, 2]), 4.0 * xb[:, 0] - 0.2], 1)
    return xb, tets, x, v, u, nb


def _body_want(pkg, xb, tets, x, v, u, nb, mu=0.5):
    tris = pkg.meshgen.tet_surface(tets)
    nodes = np.unique(tris)
    local = -np.ones(nb, dtype=np.int64); local[nodes] = np.arange(len(nodes))
    V, F = x[nodes], local[tris].astype(np.int32)
    p = (x[nb:] + DT * v[nb:]) + u
    M = pkg.Mesh(V, F)
    M.set_vertices(V)                                                              # (the arithmetic of the device's frame-start update)
    proj, sd = M.query(p)
    hit = sd > 0
    q = np.where(hit[:, None], proj, p)
    vi, _, _ = pkg.mesh_velocity_query(M, None, p, v[nodes])
    w = _np_rigid(Z9, q) + DT * vi
    z, mode = pkg.friction_query_moving(p, q, x[nb:], w, mu)
    return p, z, mode[hit], tris


def test_body_case_counts(pkg):
    _, _, modes, _ = _body_want(pkg, *_body_case(pkg))
    assert (modes == 1).sum() >= 10 and (modes == 2).sum() >= 10, [int((modes == k).sum()) for k in range(3)]


@pytest.mark.gpu
def test_body_surface_kernel_equals_host(pkg):
    """one tet body with its surface at coefficient 0.5 and 200 free nodes, one frame of one iteration: the free nodes' z bitwise the
    host composition with the frame-start x of the surface's nodes as the mesh and their frame-start v as the vertex velocities"""
    xb, tets, x, v, u, nb = _body_case(pkg)
    p, want, modes, tris = _body_want(pkg, xb, tets, x, v, u, nb)
    counts = [int((modes == k).sum()) for k in range(3)]
    print("body surface: none / stick / slip at the hits:", counts)
    assert counts[1] >= 10 and counts[2] >= 10, counts
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    b = s.add_forces(KIND["COLLISION"], np.arange(nb, len(x), dtype=np.int32), [W])
    sid = s.add_body_surface(0, nb, tris)
    s.set_collision_shapes([MESH], [[0, 0, 0, sid]])
    s.set_body_surface_friction(sid, 0.5)
    s.initialize()
    s.m_v = v.ravel()
    s.write_local(b, u=u)
    s.step(1)
    r = s.read_local(b)
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.count_nonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + ((x[nb:] + DT * v[nb:]) - want))
    st = s.body_surface_status(sid)
    assert st["updated"] == 1 and st["refused"] == 0, st
    # the surface's velocity matters, and so does its coefficient
    _, still, _, _ = _body_want(pkg, xb, tets, x, np.zeros_like(v), u, nb)
    assert np.abs(still - want).max() > 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: whole frames
# ---------------------------------------------------------------------------------------------------------------------------------
BELT = np.array([0.8, 0.0, -0.3])


def _run_belt(pkg, x, v, g, mu, vb, frames, iters):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity(g)
    s.set_collision_shapes([FLOOR], [[0, 0, 0, 0]])
    s.set_collision_friction([mu])
    s.set_collision_motion([[*vb, 0, 0, 0, 0, 0, 0]])
    s.initialize()
    s.m_v = v.ravel()
    xs, vs = [], []
    for _ in range(frames):
        s.step(iters)
        xs.append(s.m_x.reshape(-1, 3).copy()); vs.append(s.m_v.reshape(-1, 3).copy())
    return xs, vs


@pytest.mark.gpu
def test_conveyor_particles_follow_the_model(pkg):
    """130 particles, 20 frames x 20 iterations on a floor in rigid linear motion, mu 0.45: x and v within 1e-9 of the numpy recursion;
    with mu = inf particles released at rest on the floor advance vb dt a frame once in contact, to 1e-12"""
    x, v = _particle_scene()
    g = _tilt(0.25)
    mx, mv, last = _belt_particles(x, v, g, 0.45, BELT, 20, 20)
    counts = [int((last == k).sum()) for k in (-1, 1, 2)]
    print("conveyor at the last frame: airborne %d, sticking %d, slipping %d" % tuple(counts))
    assert counts[1] >= 10 and counts[2] >= 1, counts
    xs, vs = _run_belt(pkg, x, v, g, 0.45, BELT, 20, 20)
    ex = max(np.abs(a - b).max() for a, b in zip(xs, mx))
    ev = max(np.abs(a - b).max() for a, b in zip(vs, mv))
    print("conveyor: max |x - model| %.3g, |v - model| %.3g" % (ex, ev))
    assert ex <= 1e-9 and ev <= 1e-9, (ex, ev)
    # mu = inf, released at rest on the floor: 20 iterations a frame leave the release's transient behind (the tangential recursion
    # contracts by (1 + dt^2 W^2)^-20 = 1e-3 a frame from 1.7e-5 at the contact frame: below 1e-12 from the sixth frame on; the normal
    # direction settles more slowly -- the numpy recursion gives 4e-14 at the tenth frame), so the advance is asserted tangentially from
    # frame 7 on and in all three components over the last two of 12 frames
    x0 = x.copy(); x0[:, 1] = 0.0
    gdown = np.array([0.0, -G, 0.0])
    xs, _ = _run_belt(pkg, x0, np.zeros_like(x0), gdown, np.inf, BELT, 12, 20)
    ms, _, _ = _belt_particles(x0, np.zeros_like(x0), gdown, np.inf, BELT, 12, 20)
    adv, madv = np.diff(np.array(xs), axis=0), np.diff(np.array(ms), axis=0)
    err_t = np.abs(adv[6:][:, :, [0, 2]] - DT * BELT[[0, 2]]).max()
    err_all = np.abs(adv[9:] - DT * BELT).max()
    merr = np.abs(madv[9:] - DT * BELT).max()
    print("conveyor, mu = inf: max |advance - vb dt| tangential from frame 7 on %.3g, all components over the last two frames %.3g (numpy recursion %.3g)"
          % (err_t, err_all, merr))
    assert err_t <= 1e-12 and err_all <= 1e-12, (err_t, err_all)


PLATFORM_V = np.array([0.5, 0.0, 0.0])


def _carry_system(pkg):
    """the slab of test_collision_friction resting on a cube obstacle (top face y = 0, 2 x 2 wide), gravity straight down"""
    mg = pkg.meshgen
    x, tets = mg.bar(*SLAB)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    Vc, Fc = mesh("cube")
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    s.add_collision_mesh(Vc * 2.0, Fc)
    s.set_collision_shapes([MESH], [[*CUBE_T0, 0]])
    s.set_collision_friction([np.inf])
    s.mass = m
    s.x_start = x
    return s


CUBE_T0 = np.array([-0.8, -2.0, -0.8])


def _carry_frames(s, frames, iters, motion_of_frame):
    """each frame the caller translates the cube by v dt (v = motion_of_frame(f), None: the cube moves but no motion is set)"""
    t = CUBE_T0.copy()
    out = []
    for f in range(frames):
        vb = motion_of_frame(f)
        t = t + DT * (PLATFORM_V if vb is None else vb)
        s.set_collision_shapes([MESH], [[*t, 0]])
        if vb is not None:
            s.set_collision_motion([[*vb, 0, 0, 0, 0, 0, 0]])
        s.step(iters)
        out.append(s.m_x.copy())
    return out, t - CUBE_T0


def _centroid_travel(s, x):
    return (s.mass[:, None] * (x.reshape(-1, 3) - s.x_start)).sum(0) / s.mass.sum()


_carry_cache = {}


def _carry_run(pkg, with_motion, frames=40, iters=20):
    if with_motion not in _carry_cache:
        s = _carry_system(pkg)
        s.initialize()
        xs, moved = _carry_frames(s, frames, iters, (lambda f: PLATFORM_V) if with_motion else (lambda f: None))
        _carry_cache[with_motion] = (np.array(xs), _centroid_travel(s, xs[-1]), moved)
    return _carry_cache[with_motion]


@pytest.mark.gpu
def test_carry(pkg):
    """the slab on a platform that the caller translates by 0.5 dt a frame, mu = inf, 40 frames: with the matching rigid motion set, the
    slab's centroid travels nearer to the platform's travel than to zero; with the motion left at zero (the existing kernel, which
    sticks to the frame-start position in the world) nearer to zero.  Both ratios are printed."""
    _, ta, moved = _carry_run(pkg, True)
    _, tb, _ = _carry_run(pkg, False)
    ra, rb = ta[0] / moved[0], tb[0] / moved[0]
    print("carry: platform travel %.4f; slab travel / platform travel with the motion set %.4f, without %.4f" % (moved[0], ra, rb))
    assert ra > 0.5 and rb < 0.5, (ra, rb)
    assert abs(ta[1]) < 0.02 and abs(tb[1]) < 0.02                               # it stayed on the platform


def _stack_system(pkg, mu, rank=0, world=1, mode=None):
    """two slabs of test_collision_friction, one on the other; the lower one's bottom layer anchored, each slab's surface on the list,
    gravity tilted by atan 0.25 towards +x"""
    mg = pkg.meshgen
    x1, tets = mg.bar(*SLAB)
    n1 = len(x1)
    x = np.concatenate([x1, x1 + np.array([0.0, 0.1, 0.0])])
    T = np.concatenate([tets, tets + n1])
    m = np.tile(mg.lumped_tet_mass(x1, tets, 1000.0), 2)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], T, [2e4])
    s.add_forces(KIND["ANCHOR"], np.nonzero(x1[:, 1] == 0.0)[0].astype(np.int32), [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity(_tilt(0.25))
    surf = mg.tet_surface(tets)
    s.sid = [s.add_body_surface(0, n1, surf), s.add_body_surface(n1, n1, surf + n1)]
    s.set_collision_shapes([MESH, MESH], [[0, 0, 0, s.sid[0]], [0, 0, 0, s.sid[1]]])
    for i in s.sid:
        s.set_body_surface_friction(i, mu)
    if world > 1:
        s.set_shard(rank, world)
        s.set_shard_mode(mode)
    s.mass, s.x_start, s.n1 = m, x, n1
    return s


def _upper_travel(s, x):
    d = x.reshape(-1, 3)[s.n1:] - s.x_start[s.n1:]
    return float((s.mass[s.n1:] * d[:, 0]).sum() / s.mass[s.n1:].sum())


_stack_cache = {}


def _stack_frames(pkg, mu, frames=16, iters=20):
    if mu not in _stack_cache:
        s = _stack_system(pkg, mu)
        s.initialize()
        xs = []
        for _ in range(frames):
            s.step(iters)
            xs.append(s.m_x.copy())
        st = [s.body_surface_status(i) for i in s.sid]
        assert all(q["refused"] == 0 and q["updated"] == frames for q in st), st
        _stack_cache[mu] = (np.array(xs), _upper_travel(s, xs[-1]))
    return _stack_cache[mu]


@pytest.mark.gpu
def test_stack_travel_decreases_with_surface_friction(pkg):
    """the upper slab's travel along the slope after 16 frames x 20 iterations (a free slide of 0.13, a third of the lower slab's length:
    the upper one stays supported) for surface coefficients 0, 0.125, 0.5: strictly decreasing; no frame's surface update refused.
    The ratios are printed."""
    t = {mu: _stack_frames(pkg, mu)[1] for mu in (0.0, 0.125, 0.5)}
    print("stack: upper slab travel mu 0 -> %.6f, 0.125 -> %.6f, 0.5 -> %.6g; ratio travel(0.125) / travel(0) = %.4f, travel(0.5) / travel(0) = %.3g"
          % (t[0.0], t[0.125], t[0.5], t[0.125] / t[0.0], t[0.5] / t[0.0]))
    assert t[0.0] > t[0.125] > t[0.5], t


@pytest.mark.gpu
def test_launch_modes_bitwise(pkg, monkeypatch):
    """the carry scene with the platform's speed halved from frame 6 on, and the stack with the surfaces' coefficient going 0 -> 0.5 -> 0
    at frames 3 and 6, under ADMM_HIP_GRAPH 0 / 1 and ADMM_HIP_FRAME_GRAPH 0 / 1: bitwise equal frames"""
    res = []
    for env in ({"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "1"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        s = _carry_system(pkg)
        s.initialize()
        xs, _ = _carry_frames(s, 10, 10, lambda f: PLATFORM_V if f < 6 else 0.5 * PLATFORM_V)
        t = _stack_system(pkg, 0.0)
        t.initialize()
        ys = []
        for f in range(9):
            if f in (3, 6):
                for i in t.sid:
                    t.set_body_surface_friction(i, 0.5 if f == 3 else 0.0)
            t.step(10)
            ys.append(t.m_x.copy())
        res.append((xs, ys, s.graph_state()["graph_launches"], t.graph_state()["graph_launches"]))
    for r in res[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r[0], res[0][0])) and all(np.array_equal(a, b) for a, b in zip(r[1], res[0][1]))
    assert res[0][2] == 0 and res[0][3] == 0 and res[1][2] > 0 and res[1][3] > 0
    assert np.abs(res[0][1][5] - res[0][1][2]).max() > 0


@pytest.mark.gpu
def test_stack_two_subtree_shards(pkg, monkeypatch):
    """the stack at surface coefficient 0.125 as two subtree shards on one GPU: the ranks bitwise equal, within 1e-9 of one rank"""
    from test_sharding import _run_sharded, _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    frames, iters = 8, 20
    ref = _stack_system(pkg, 0.125)
    ref.initialize()
    shards = [_stack_system(pkg, 0.125, rank=r, world=2, mode="subtree") for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    assert all(s.info()["n_elems_local"] > 0 for s in shards)
    b = np.random.default_rng(2).normal(size=3 * ref.n_nodes)
    out = _run_sharded(shards, frames, iters, b)
    refx = []
    for _ in range(frames):
        ref.step(iters)
        refx.append(ref.m_x.copy())
    for r in range(2):
        _, xs, vs = out[r]
        for f in range(frames):
            assert np.abs(xs[f] - refx[f]).max() < 1e-9, (r, f, np.abs(xs[f] - refx[f]).max())
        assert all(np.array_equal(p, q) for p, q in zip(xs, out[0][1])) and np.array_equal(vs, out[0][2])
    assert _upper_travel(ref, refx[-1]) > 1e-4                                     # it did slide


@pytest.mark.gpu
def test_stack_residual_tracking_leaves_x_alone(pkg):
    """tracking reads z in passes of its own for the collision batches: the frames are bitwise the same with it on"""
    frames, iters = 10, 20
    plain, _ = _stack_frames(pkg, 0.125)
    s = _stack_system(pkg, 0.125)
    s.initialize()
    s.enable_residuals(True)
    for f in range(frames):
        s.step(iters)
        assert np.array_equal(s.m_x, plain[f]), f
    r, d, k = s.residuals()
    assert k == iters and np.isfinite(r).all() and np.isfinite(d).all() and r.max() > 0


@pytest.mark.gpu
def test_class_api_moving_friction(pkg, tmp_path):
    """CollisionShape::lin_velocity (mode 0, the carry scene) and CollisionBody::surface_friction (mode 1, the stack) through
    admm::System: the frames bitwise equal to the C ABI's"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_moving_friction", pkg)
    mg = pkg.meshgen
    x, tets = mg.bar(*SLAB)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    surf = mg.tet_surface(tets)
    Vc, Fc = mesh("cube")
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(tets), len(surf), len(Vc), len(Fc)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f); tets.astype(np.int32).tofile(f); surf.astype(np.int32).tofile(f)
        (Vc * 2.0).astype(np.float64).tofile(f); Fc.astype(np.int32).tofile(f)
        np.concatenate([CUBE_T0, PLATFORM_V, _tilt(0.25), [0.125]]).tofile(f)
    frames = 12
    want = _carry_run(pkg, True)[0]
    r = subprocess.run([exe, "0", inp, out, str(frames), "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(out).reshape(frames, -1)
    assert np.array_equal(got, want[:frames]), np.abs(got - want[:frames]).max()
    want = _stack_frames(pkg, 0.125)[0]
    r = subprocess.run([exe, "1", inp, out, str(frames), "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(out).reshape(frames, -1)
    assert np.array_equal(got, want[:frames]), np.abs(got - want[:frames]).max()
