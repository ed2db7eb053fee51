"""Coulomb friction at collision contacts (admm_hip_set_collision_friction): the rule's host evaluation (admm_hip_friction_query) against
an extended-precision numpy restatement, the argument checks, and on the GPU: the friction kernel bit for bit against the host routine
(analytic shapes, meshes, owners), all-zero coefficients as the frictionless path, free particles and a tet slab over whole frames against
a numpy particle recursion and against closed forms, launch modes, subtree shards, residual tracking and the class API.

No reference counterpart: the expected values come from numpy in here."""

import subprocess

import numpy as np
import pytest

from checkers import KIND
from test_collision_mesh import FLOOR, MESH, SPHERE, _bar_scene, _np_floor, _np_sphere, mesh

CYLINDER = 2
DT, W = 0.02, 32.0
G = 9.8


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule in numpy (any float type), the particle recursion
# ---------------------------------------------------------------------------------------------------------------------------------
def _np_friction(p, po, x0, mu):
    """the rule of include/admm_hip.h, row by row; the dtype of p decides the precision -> (result, mode, tl, lim)"""
    p, po, x0 = np.asarray(p), np.asarray(po), np.asarray(x0)
    mu = np.broadcast_to(np.asarray(mu, dtype=p.dtype), (len(p),))
    d = po - p
    depth = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    on = (mu > 0) & (depth > 0)
    safe = np.where(on, depth, 1)
    n = d / safe[:, None]
    r = po - x0
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
    mode = np.where(stick, 1, np.where(slip, 2, 0)).astype(np.int32)
    return out, mode, tl, lim


def _tilt(slope):
    """gravity of size G tilted by atan(slope) towards +x over a floor y = const"""
    th = np.arctan(slope)
    return np.array([G * np.sin(th), -G * np.cos(th), 0.0])


def _particles(x, v, g, mu_of_frame, frames, iters, m=1.0, cy=0.0):
    """free particles of mass m, one collision element each (weight W) against the floor y = cy: the ADMM recursion of admm_hip_step
    (prologue, `iters` times local step / right-hand side / solve, epilogue) in numpy -> (x, v per frame, mode of the last projection:
    -1 airborne, 1 stick, 2 slip, 0 pushed without friction)"""
    x, v = x.copy(), v.copy()
    u = np.zeros_like(x)
    k = DT * DT * W * W
    xs, vs, last = [], [], None
    for f in range(frames):
        mu = mu_of_frame(f)
        v = v + DT * g
        xbar = x + DT * v
        xc = xbar.copy()
        for _ in range(iters):
            p = xc + u
            z = _np_floor(p, cy)
            hit = (z != p).any(1)
            z, mode, _, _ = _np_friction(p, z, x, mu)
            last = np.where(hit, mode, -1)
            u = u + (xc - z)
            xc = (m * xbar + k * (z - u)) / (m + k)
        v = (xc - x) / DT
        x = xc
        xs.append(x.copy()); vs.append(v.copy())
    return xs, vs, last


def _np_cylinder(p, c, R):
    d0, d1 = p[:, 0] - c[0], p[:, 1] - c[1]
    nrm = np.sqrt(d0 * d0 + (d1 * d1 + 0.0))
    hit = R - nrm > 0
    q = p.copy()
    q[hit, 0] = (c[0] + R * (d0[hit] / nrm[hit])) + 0.0
    q[hit, 1] = (c[1] + R * (d1[hit] / nrm[hit])) + 0.0
    return q


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_friction_query_vs_longdouble(pkg):
    """4096 random cases, every coordinate in [-2, 2], depth >= 1e-3, mu from {0, 0.1, 0.5, 2, inf}; a case whose |t| is within 1e-6 of
    the cone's radius is drawn again (at most 1 % of them), so that the mode is decided away from rounding.  Modes exact; the result
    within 64 eps max(1, |p|, |x0|): under 32 roundings, each relative to a quantity below that scale, the normalisation well
    conditioned by the depth floor."""
    n = 4096
    rng = np.random.default_rng(11)
    mus = np.array([0.0, 0.1, 0.5, 2.0, np.inf])

    def draw(k):
        return rng.uniform(-2, 2, (k, 3)), rng.uniform(-2, 2, (k, 3)), rng.uniform(-2, 2, (k, 3)), mus[rng.integers(0, 5, k)]
    p, po, x0, mu = draw(n)
    redrawn = 0
    for _ in range(20):
        L = np.longdouble
        _, _, tl, lim = _np_friction(p.astype(L), po.astype(L), x0.astype(L), mu.astype(L))
        depth = np.linalg.norm(po - p, axis=1)
        bad = np.nonzero((np.abs(tl - lim) < 1e-6) | (depth < 1e-3))[0]
        if bad.size == 0:
            break
        redrawn += bad.size
        p[bad], po[bad], x0[bad], mu[bad] = draw(bad.size)
    assert bad.size == 0 and redrawn <= n // 100, redrawn
    L = np.longdouble
    want, wmode, _, _ = _np_friction(p.astype(L), po.astype(L), x0.astype(L), mu.astype(L))
    got, mode = pkg.friction_query(p, po, x0, mu)
    assert np.array_equal(mode, wmode)
    for k in range(3):
        assert (mode == k).sum() >= 100, (k, (mode == k).sum())
    tol = 64 * np.finfo(np.float64).eps * np.maximum(1.0, np.maximum(np.linalg.norm(p, axis=1), np.linalg.norm(x0, axis=1)))
    err = np.abs((got.astype(L) - want).astype(np.float64)).max(1)
    print("friction_query vs longdouble: max error %.3g, smallest bound %.3g, worst ratio %.3g" % (err.max(), tol.min(), (err / tol).max()))
    assert (err <= tol).all(), (err / tol).max()
    assert np.array_equal(got[mu == 0], po[mu == 0]) and not mode[mu == 0].any()          # mu = 0: p_out untouched, mode none
    assert (mode[np.isinf(mu)] == 1).all()                                                  # mu = inf always sticks
    got, mode = pkg.friction_query(p, p, x0, np.where(mu > 0, mu, 0.5))                     # depth == 0 likewise
    assert np.array_equal(got, p) and not mode.any()


def _expect(pkg, call, *words):
    with pytest.raises(pkg.AdmmHipError) as e:
        call()
    for w in words:
        assert w in str(e.value), str(e.value)


def test_friction_argument_checks(pkg):
    """a host-only context: what admm_hip_set_collision_friction refuses, what finalize refuses, and the coefficients a new shape list
    keeps (the same length) or loses (another length), seen through which lists are then accepted"""
    mg = pkg.meshgen
    xb, tets = mg.bar(1, 1, 1)
    x = np.concatenate([xb, np.random.default_rng(0).uniform(-1, 2, size=(40, 3))])
    s = pkg.System(device_id=-1)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    sid = s.add_body_surface(0, len(xb), mg.tet_surface(tets))
    floor, sph, body = [0, -1, 0, 0], [0.5, 0.5, 0.5, 0.2], [0, 0, 0, sid]
    s.set_collision_shapes([FLOOR, SPHERE, MESH], [floor, sph, body])
    _expect(pkg, lambda: s.set_collision_friction([-0.1, 0, 0]), "error 1", "shape 0", "negative")
    _expect(pkg, lambda: s.set_collision_friction([0, np.nan, 0]), "error 1", "shape 1")
    _expect(pkg, lambda: s.set_collision_friction([0.1, 0.2]), "error 1", "2 coefficients", "3 entries")
    _expect(pkg, lambda: s.set_collision_friction([0.1, 0.2, 0.3]), "error 1", "shape 2", "body surface")
    s.set_collision_friction([0.5, np.inf, 0.0])                                    # +inf is a coefficient
    # the same length keeps the coefficients: the body surface moves to entry 1, where inf is set -> finalize refuses, naming it
    s.set_collision_shapes([FLOOR, MESH, SPHERE], [floor, body, sph])
    _expect(pkg, s.initialize, "error 1", "shape 1", "body surface")
    # another length zeroes them: back at three entries the same list is accepted by finalize
    s.set_collision_shapes([FLOOR, MESH], [floor, body])
    s.set_collision_shapes([FLOOR, MESH, SPHERE], [floor, body, sph])
    s.initialize()
    # after finalize: the call's own checks again, and a kept coefficient that would land on the body surface is refused by set_collision_shapes
    _expect(pkg, lambda: s.set_collision_friction([0, 0.1, 0]), "shape 1", "body surface")
    _expect(pkg, lambda: s.set_collision_friction([0, 0, -1.0]), "shape 2", "negative")
    _expect(pkg, lambda: s.set_collision_friction([0.0]), "1 coefficients", "3 entries")
    s.set_collision_friction([0.3, 0, 0.2])
    _expect(pkg, lambda: s.set_collision_shapes([MESH, FLOOR, SPHERE], [body, floor, sph]), "shape 0", "body surface")
    s.set_collision_shapes([SPHERE, MESH, FLOOR], [sph, body, floor])               # (0.3, 0, 0.2) kept: the body's entry has 0
    s.set_collision_shapes([FLOOR], [floor])
    s.set_collision_shapes([MESH, FLOOR, SPHERE], [body, floor, sph])               # zeroed by the change of length: accepted now


def test_particle_model_closed_forms():
    """the numpy recursion the GPU tests compare with, at 100 iterations a frame, against what Coulomb friction gives a particle in
    closed form: on a slope of tan = 0.5 the travel scales with 1 - mu / tan below the slope's tangent and is zero above it; on a flat
    floor a particle of speed 1 under mu = 0.5 loses mu g dt a frame, v_k = 1 - 0.098 k for k <= 10, and stops after
    dt * sum v_k = 0.02 * (10 - 0.098 * 55) = 0.0922 (the continuous v0^2 / (2 mu g) - v0 dt / 2 = 0.0920).  Guards the reference."""
    z3 = np.zeros((1, 3))
    g = _tilt(0.5)

    def travel(mu):
        xs, _, _ = _particles(z3, z3, g, lambda f: mu, 40, 100)
        return xs[-1][0]
    t0 = travel(0.0)
    a, T = G * np.sin(np.arctan(0.5)), 40 * DT
    assert abs(t0[0] - 0.5 * a * T * (T + DT)) <= 1e-8 * t0[0] and abs(t0[1]) <= 1e-12
    assert abs(travel(0.25)[0] / t0[0] / 0.5 - 1) <= 1e-8
    assert abs(travel(0.45)[0] / t0[0] / 0.1 - 1) <= 1e-8
    assert np.abs(travel(0.55)).max() <= 1e-12 and np.abs(travel(1.0)).max() <= 1e-12
    xs, vs, _ = _particles(z3, np.array([[1.0, 0, 0]]), np.array([0, -G, 0.0]), lambda f: 0.5, 40, 100)
    assert abs(xs[-1][0, 0] - 0.0922) <= 1e-6 and np.abs(vs[-1]).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the host routine
# ---------------------------------------------------------------------------------------------------------------------------------
def _points_system(pkg, X0, types, params, mu, meshes=(), owner=None):
    """free nodes at X0 that each carry one collision element"""
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    n = len(X0)
    s.add_nodes(X0.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
    for V, F in meshes:
        s.add_collision_mesh(V, F)
    if owner:
        s.set_collision_mesh_owner(*owner)
    s.set_collision_shapes(types, params)
    s.set_collision_friction(mu)
    s.initialize()
    return s, b


def _compose(pkg, p, x0, pushes):
    """the list's pushes in order, friction after each; -> (z, modes of the applications that moved a point)"""
    modes = []
    for push, mu in pushes:
        q = push(p)
        moved = (q != p).any(1)
        q, mode = pkg.friction_query(p, q, x0, mu)
        modes.append(mode[moved])
        p = q
    return p, np.concatenate(modes)


def _kernel_case(n, seed):
    rng = np.random.default_rng(seed)
    dx = rng.uniform(-1, 1, (n, 3))
    x0 = dx + 0.15 * rng.normal(size=(n, 3))          # the nodes as added: the frame start
    u = 0.2 * rng.normal(size=(n, 3))
    near = rng.uniform(size=n) < 0.5                  # half of them start the frame close to the candidate: small tangential parts, which stick
    x0[near] = (dx + u)[near] + 0.03 * rng.normal(size=(int(near.sum()), 3))
    return dx, x0, u


@pytest.mark.gpu
def test_kernel_equals_host_routine_analytic(pkg):
    """200 nodes (three full 64-lane blocks and a partial one), [floor 0.3, sphere 0, sphere 0.7, z-cylinder inf]: z and u bitwise"""
    n = 200
    dx, x0, u = _kernel_case(n, 3)
    cy, c1, R1, c2, R2, cc, Rc = -0.4, np.array([0.5, 0.2, 0.0]), 0.6, np.array([-0.5, 0.3, 0.2]), 0.6, np.array([0.0, 0.6, 0.0]), 0.4
    mu = [0.3, 0.0, 0.7, np.inf]
    s, b = _points_system(pkg, x0, [FLOOR, SPHERE, SPHERE, CYLINDER], [[0, cy, 0, 0], [*c1, R1], [*c2, R2], [*cc, Rc]], mu)
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    want, modes = _compose(pkg, dx + u, x0, [(lambda p: _np_floor(p, cy), mu[0]), (lambda p: _np_sphere(p, c1, R1), mu[1]),
                                             (lambda p: _np_sphere(p, c2, R2), mu[2]), (lambda p: _np_cylinder(p, cc, Rc), mu[3])])
    counts = [int((modes == k).sum()) for k in range(3)]
    print("analytic shapes: none / stick / slip among the pushes:", counts)
    assert min(counts) >= 10, counts
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.count_nonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))


@pytest.mark.gpu
def test_kernel_equals_host_routine_meshes(pkg):
    """[floor 0.2, cube 0.5, ico2 0.5], the cube owned by the first 60 nodes: expected values from mesh_query and friction_query, bitwise;
    an owner's node inside the cube is not pushed by it"""
    n = 200
    dx, x0, u = _kernel_case(n, 4)
    Vc, Fc = mesh("cube")
    Vi, Fi = mesh("ico2")
    Vi = Vi * 0.7
    tc, ti, cy = np.array([-0.6, -0.3, -0.5]), np.array([0.4, 0.3, 0.2]), -0.5
    mu = [0.2, 0.5, 0.5]
    own = np.arange(n) < 60
    s, b = _points_system(pkg, x0, [FLOOR, MESH, MESH], [[0, cy, 0, 0], [*tc, 0], [*ti, 1]], mu, meshes=[(Vc, Fc), (Vi, Fi)], owner=(0, 0, 60))
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)

    def mesh_push(V, F, t, skip=None):
        def push(p):
            proj, sd = pkg.mesh_query(V, F, p, t)
            hit = sd > 0
            if skip is not None:
                hit &= ~skip
            return np.where(hit[:, None], proj, p)
        return push
    want, modes = _compose(pkg, dx + u, x0, [(lambda p: _np_floor(p, cy), mu[0]), (mesh_push(Vc, Fc, tc, own), mu[1]), (mesh_push(Vi, Fi, ti), mu[2])])
    counts = [int((modes == k).sum()) for k in range(3)]
    print("meshes: none / stick / slip among the pushes:", counts)
    assert counts[1] >= 10 and counts[2] >= 10, counts
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.count_nonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))
    # owners inside their own cube (and touched by nothing else) keep their candidate
    p = dx + u
    _, sd = pkg.mesh_query(Vc, Fc, p, tc)
    _, sdi = pkg.mesh_query(Vi, Fi, p, ti)
    free = own & (sd > 0) & (p[:, 1] >= cy) & (sdi <= 0)
    assert free.sum() >= 3, free.sum()
    assert np.array_equal(r["z"][free], p[free])
    assert ((sd > 0) & ~own).sum() >= 10                                         # and the others are pushed out of it


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: whole frames
# ---------------------------------------------------------------------------------------------------------------------------------
BAR_FLOOR = -0.03


def _bar(pkg):
    """the cantilever of test_collision_mesh over a floor and a sphere close enough under it to be reached within five frames"""
    return _bar_scene(pkg, [], lambda f: ([FLOOR, SPHERE], [[0, BAR_FLOOR, 0, 0], [0.15, -0.21, 1.0, 0.2]]))


def _bar_frames(s, frames, iters=10):
    out = []
    for _ in range(frames):
        s.step(iters)
        loc = [s.read_local(b) for b in range(3)]
        out.append((s.m_x.copy(), s.m_v.copy(), [q["u"].copy() for q in loc], [q["z"].copy() for q in loc]))
    return out


def _same(a, b):
    return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))
               and all(np.array_equal(p, q) for p, q in zip(a[3], b[3])) for a, b in zip(a, b))


@pytest.mark.gpu
def test_zero_coefficients_are_the_frictionless_path(pkg):
    """(a) never calls the new entry, (b) sets zeros, (c) runs two frames with friction after finalize and goes back to zeros (the
    captured graphs are dropped twice): x, v, u, z of the 6 x 4 x 24 bar over 5 frames bitwise equal, (c) from the same state"""
    a = _bar(pkg); a.initialize()
    x_start = a.m_x.copy()
    fa = _bar_frames(a, 5)
    zc = fa[-1][3][2]                                                          # the collision batch's z of the last iteration
    assert (zc[:, 1] == BAR_FLOOR).any() and fa[-1][0].reshape(-1, 3)[:, 1].min() < -0.02      # the bar did reach the floor
    b = _bar(pkg); b.set_collision_friction([0.0, 0.0]); b.initialize()
    assert _same(fa, _bar_frames(b, 5))
    c = _bar(pkg); c.initialize()
    c.set_collision_friction([0.5, 0.25])
    _bar_frames(c, 2)
    assert c.graph_state()["graph_launches"] > 0
    c.set_collision_friction([0.0, 0.0])
    c.m_x = x_start; c.m_v = np.zeros_like(x_start)
    for bt in range(3):
        c.write_local(bt, u=np.zeros_like(fa[0][2][bt]))
    assert _same(fa, _bar_frames(c, 5))
    assert c.graph_state()["graph_launches"] > 0


def _particle_scene(n=130, seed=5):
    """130 free particles over the floor y = 0 under gravity tilted by atan 0.25 (below mu = 0.45: what rests, sticks): a third high in
    the air, a third on the floor and slow, a third on the floor and fast or just above it"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3)); v = np.zeros((n, 3))
    x[:, 0] = rng.uniform(-1, 1, n); x[:, 2] = rng.uniform(-1, 1, n)
    air, slow = np.arange(n) < 45, (np.arange(n) >= 45) & (np.arange(n) < 90)
    fast = ~air & ~slow
    x[air, 1] = rng.uniform(1.5, 3.0, air.sum())
    v[air] = rng.normal(size=(air.sum(), 3))
    ang = rng.uniform(0, 2 * np.pi, n)
    sp = np.where(slow, rng.uniform(0.0, 0.3, n), rng.uniform(2.0, 3.5, n))
    v[~air, 0] = (sp * np.cos(ang))[~air]; v[~air, 2] = (sp * np.sin(ang))[~air]
    x[fast, 1] = np.where(rng.uniform(size=fast.sum()) < 0.5, 0.0, rng.uniform(0.0, 0.05, fast.sum()))
    return x, v


def _run_particles(pkg, x, v, g, mu_of_frame, frames, iters):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity(g)
    s.set_collision_shapes([FLOOR], [[0, 0, 0, 0]])
    s.set_collision_friction([mu_of_frame(0)])
    s.initialize()
    assert s.info()["dense_solve"] == 1
    s.m_v = v.ravel()
    xs, vs = [], []
    for f in range(frames):
        if f and mu_of_frame(f) != mu_of_frame(f - 1):
            s.set_collision_friction([mu_of_frame(f)])
        s.step(iters)
        xs.append(s.m_x.reshape(-1, 3).copy()); vs.append(s.m_v.reshape(-1, 3).copy())
    return xs, vs, s.graph_state()


@pytest.mark.gpu
def test_free_particles_follow_the_model(pkg, monkeypatch):
    """130 particles (the dense solve), 20 frames x 20 iterations, floor mu 0.45: x and v within 1e-9 of the numpy recursion (the bound of
    paths without a truncated minimiser), in every launch mode bitwise the same, and again with the coefficient
    changed between frames 10 and 11 (the coefficients live in the shape table that a captured graph reads)"""
    x, v = _particle_scene()
    g = _tilt(0.25)
    frames, iters = 20, 20
    const = lambda f: 0.45
    change = lambda f: 0.45 if f < 10 else 0.1
    model = {}
    for name, fn in (("const", const), ("change", change)):
        model[name] = _particles(x, v, g, fn, frames, iters)
    last = model["const"][2]
    counts = [int((last == k).sum()) for k in (-1, 1, 2)]
    print("particles at the last frame: airborne %d, sticking %d, slipping %d" % tuple(counts))
    assert min(counts) >= 20, counts
    assert np.abs(model["const"][0][-1] - model["change"][0][-1]).max() > 1e-3          # the change matters
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {"ADMM_HIP_LOCAL_MULTI": "0"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        for name, fn in (("const", const), ("change", change)):
            xs, vs, gs = _run_particles(pkg, x, v, g, fn, frames, iters)
            ex = max(np.abs(a - b).max() for a, b in zip(xs, model[name][0]))
            ev = max(np.abs(a - b).max() for a, b in zip(vs, model[name][1]))
            print("particles %s %s: max |x - model| %.3g, |v - model| %.3g, graph launches %d" % (env, name, ex, ev, gs["graph_launches"]))
            assert ex <= 1e-9 and ev <= 1e-9, (env, name, ex, ev)
            res[(tuple(env.items()), name)] = (xs, vs, gs)
    keys = [k for k in res if k[1] == "const"]
    for name in ("const", "change"):
        first = res[(keys[0][0], name)]
        for k in keys[1:]:
            other = res[(k[0], name)]
            assert all(np.array_equal(p, q) for p, q in zip(first[0], other[0])) and all(np.array_equal(p, q) for p, q in zip(first[1], other[1])), (k, name)
    assert res[((("ADMM_HIP_GRAPH", "0"),), "const")][2]["graph_launches"] == 0
    assert res[((("ADMM_HIP_GRAPH", "1"),), "change")][2]["graph_launches"] > 0


SLAB = (8, 2, 8)
SLAB_SLOPE = 0.25
_slab_cache = {}


def _slab_system(pkg, mu, rank=0, world=1, mode=None):
    """a linear-strain tet slab 8 x 2 x 8 (0.4 x 0.1 x 0.4) lying on the floor y = 0, gravity tilted by atan 0.25 towards +x"""
    mg = pkg.meshgen
    x, tets = mg.bar(*SLAB)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity(_tilt(SLAB_SLOPE))
    s.set_collision_shapes([FLOOR], [[0, 0, 0, 0]])
    if mu is not None:
        s.set_collision_friction([mu])
    if world > 1:
        s.set_shard(rank, world)
        s.set_shard_mode(mode)
    s.mass = m
    return s


def _slab_frames(pkg, mu, frames=40, iters=20):
    if mu not in _slab_cache:
        s = _slab_system(pkg, mu)
        s.initialize()
        out = []
        for _ in range(frames):
            s.step(iters)
            out.append(s.m_x.copy())
        out = np.array(out)
        out.setflags(write=False)
        _slab_cache[mu] = (out, s.mass)
    return _slab_cache[mu]


def _travel(pkg, mu):
    xs, m = _slab_frames(pkg, mu)
    x0, _ = pkg.meshgen.bar(*SLAB)
    return float((m * (xs[-1].reshape(-1, 3)[:, 0] - x0[:, 0])).sum() / m.sum())


@pytest.mark.gpu
def test_slab_travel_decreases_with_friction(pkg):
    """the slab's centre of mass along the slope after 40 frames x 20 iterations for mu in {0, 0.125, 0.5}: strictly decreasing, and at
    0.5 (twice the slope's tangent) at most a tenth of the frictionless travel -- a wide margin: the particle model sticks to 2e-5 of
    the free travel at 20 iterations.  The ratio at 0.125, where the particle model gives 0.5, is printed."""
    t = {mu: _travel(pkg, mu) for mu in (0.0, 0.125, 0.5)}
    free = 0.5 * G * np.sin(np.arctan(SLAB_SLOPE)) * 0.8 * 0.82
    print("slab travel: mu 0 -> %.6f (a particle: %.6f), 0.125 -> %.6f, 0.5 -> %.6g; ratio travel(0.125) / travel(0) = %.4f, travel(0.5) / travel(0) = %.3g"
          % (t[0.0], free, t[0.125], t[0.5], t[0.125] / t[0.0], t[0.5] / t[0.0]))
    assert t[0.0] > t[0.125] > t[0.5]
    assert t[0.5] <= 0.1 * t[0.0]


@pytest.mark.gpu
def test_slab_two_subtree_shards(pkg, monkeypatch):
    """the slab at mu = 0.125 as two subtree shards on one GPU (every rank holds the full frame-start x): the ranks bitwise equal,
    within 1e-9 of the one-rank run"""
    from test_sharding import _run_sharded, _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    frames, iters = 8, 20
    ref = _slab_system(pkg, 0.125)
    ref.initialize()
    shards = [_slab_system(pkg, 0.125, rank=r, world=2, mode="subtree") for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    assert all(s.info()["n_elems_local"] > 0 for s in shards)
    assert sum(s.info()["n_elems_local"] for s in shards) == ref.info()["n_elems_total"]
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
    x0, _ = pkg.meshgen.bar(*SLAB)
    assert (refx[-1].reshape(-1, 3)[:, 0] - x0[:, 0]).mean() > 1e-3                  # it did slide


@pytest.mark.gpu
def test_slab_residual_tracking_leaves_x_alone(pkg):
    """tracking reads z in passes of its own for the collision batches: the frames are bitwise the same with it on"""
    frames, iters = 10, 20
    plain, _ = _slab_frames(pkg, 0.125)
    s = _slab_system(pkg, 0.125)
    s.initialize()
    s.enable_residuals(True)
    for f in range(frames):
        s.step(iters)
        assert np.array_equal(s.m_x, plain[f]), f
    r, d, k = s.residuals()
    assert k == iters and np.isfinite(r).all() and np.isfinite(d).all() and r.max() > 0


@pytest.mark.gpu
def test_class_api_friction(pkg, tmp_path):
    """CollisionFloor::friction = 0.125 through admm::System: the slab's frames bitwise equal to the C ABI's; a user-written shape with
    a coefficient makes initialize fail with a message"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_friction", pkg)
    mg = pkg.meshgen
    x, tets = mg.bar(*SLAB)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        surf = mg.tet_surface(tets)
        np.array([len(x), len(tets), len(surf)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f); tets.astype(np.int32).tofile(f); surf.astype(np.int32).tofile(f)
        np.concatenate([_tilt(SLAB_SLOPE), [0.125]]).tofile(f)
    want, _ = _slab_frames(pkg, 0.125)
    frames = 12
    r = subprocess.run([exe, "0", inp, out, str(frames), "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(out).reshape(frames, -1)
    assert np.array_equal(got, want[:frames]), np.abs(got - want[:frames]).max()
    r = subprocess.run([exe, "1", inp, out, "1", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "friction" in r.stderr and "projects on the host" in r.stderr, r.stderr
    r = subprocess.run([exe, "2", inp, out, "1", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "CollisionBody" in r.stderr and "friction" in r.stderr, (r.returncode, r.stderr)
