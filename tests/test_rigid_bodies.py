"""Rigid bodies in the collision list, moved by their contacts on the GPU (System.add_rigid_body, admm_hip_add_rigid_body;
csrc/rigid.hpp).

CPU (no GPU, host-only contexts): rigid_query bit for bit against a plain Python restatement of rigid.hpp's order, and stage by stage
against long double within bounds derived from the operation counts; the rotation's quality over 1000 torque-free frames; free fall;
every refusal and the order of the checks.
GPU: the device bit for bit against the rule applied from outside (rigid_state -> step -> entry_resultants(pivot = c) -> rigid_query)
on three scenes, together with a twin context without bodies that is moved by the setters; a stale upload of the host's table healed
by the next step; launch modes and solver options; off is off; a checkpoint; the behaviour the feature exists for; the class mirror."""

import math

import numpy as np
import pytest

from checkers import KIND
from test_body_collision import _two_bars, _with_bodies, _refused, DT, MESH, FLOOR
from test_surface_reaction import _cube

ADMM_ERR_ARG, ADMM_ERR_HIP, ADMM_ERR_STATE, ADMM_ERR_UNSUPPORTED = 1, 2, 3, 4
SPHERE, CYLINDER, BOX = 1, 2, 4
U = 2.0 ** -53
LD = np.longdouble
DEPTH = 1e-10


def gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule, restated (csrc/rigid.hpp's header comment, operation by operation, on Python floats)
# ---------------------------------------------------------------------------------------------------------------------------------
def _invert(J):
    a, b, c, d, e, f = (float(v) for v in J)
    C0, C1, C2 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * C0 + (b * C1 + c * C2)
    return [C0 / det, C1 / det, C2 / det, (a * f - c * c) / det, (b * c - a * e) / det, (a * d - b * b) / det]


def _rotation(q):
    w, x, y, z = (float(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]


def _omega(R, J, L):
    a = [R[j] * L[0] + (R[3 + j] * L[1] + R[6 + j] * L[2]) for j in range(3)]
    b = [J[0] * a[0] + (J[1] * a[1] + J[2] * a[2]), J[1] * a[0] + (J[3] * a[1] + J[4] * a[2]), J[2] * a[0] + (J[4] * a[1] + J[5] * a[2])]
    return [R[3 * j] * b[0] + (R[3 * j + 1] * b[1] + R[3 * j + 2] * b[2]) for j in range(3)]


def _turn(q, om, dt):
    q = [float(v) for v in q]
    hd = dt / 2.0
    h = [hd * om[j] for j in range(3)]
    s = math.sqrt(1.0 + (h[0] * h[0] + (h[1] * h[1] + h[2] * h[2])))
    dw, dx, dy, dz = 1.0 / s, h[0] / s, h[1] / s, h[2] / s
    p = [dw * q[0] - (dx * q[1] + (dy * q[2] + dz * q[3])),
         dw * q[1] + (dx * q[0] + (dy * q[3] - dz * q[2])),
         dw * q[2] + (dy * q[0] + (dz * q[1] - dx * q[3])),
         dw * q[3] + (dz * q[0] + (dx * q[2] - dy * q[1]))]
    n = math.sqrt(p[0] * p[0] + (p[1] * p[1] + (p[2] * p[2] + p[3] * p[3])))
    return [v / n for v in p], p


def _restate(K, S, row, dt):
    """-> dict of every field of the new record"""
    Ji = _invert(K["inertia"])
    F = [-float(row[j]) for j in range(3)]; tau = [-float(row[3 + j]) for j in range(3)]
    m = float(K["mass"])
    v = [float(S.v[j]) + dt * (F[j] / m + float(K["accel"][j])) for j in range(3)]
    L = [float(S.L[j]) + dt * tau[j] for j in range(3)]
    R = _rotation(S.q)
    om = _omega(R, Ji, L)
    c = [float(S.c[j]) + dt * v[j] for j in range(3)]
    q, _ = _turn(S.q, om, dt)
    follows = K["type"] in (SPHERE, MESH)
    par = [float(K["par0"][j]) + (c[j] - float(K["c0"][j])) if follows else float(K["par0"][j]) for j in range(3)] + [float(K["par0"][3])]
    return dict(c=c, q=q, v=v, L=L, omega=om, R=_rotation(q), par=par, F=F, tau=tau)


def _state(pkg, c, q, v, L, entry=0):
    r = pkg.RigidStateRecord()
    r.c[:] = list(c); r.q[:] = list(q); r.v[:] = list(v); r.L[:] = list(L); r.entry = entry
    return pkg.RigidState(r)


def _unit(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def _spd(rng, scale):
    A = rng.normal(size=(3, 3))
    M = (A @ A.T + 0.3 * np.eye(3)) * scale
    return [M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]]


def _cases(rng, n):
    out = []
    for k in range(n):
        ty = (SPHERE, BOX, MESH)[k % 3]
        J = _spd(rng, 10.0 ** rng.integers(-3, 1)) if k % 4 else [0.01, 0.0, 0.0, 0.04, 0.0, 0.09]      # every fourth: diagonal, anisotropic
        K = dict(type=ty, mass=float(10.0 ** rng.uniform(-1, 1)), inertia=J, accel=rng.normal(size=3) * 9.8, c0=rng.normal(size=3), par0=rng.normal(size=4))
        L = rng.normal(size=3) * 10.0 ** rng.integers(-3, 1)
        row = rng.normal(size=6) * 10.0 ** rng.integers(-2, 3)
        if k % 5 == 1:
            L = np.zeros(3); row[3:] = 0.0                                   # omega = 0
        if k % 5 == 2:
            row[3:] = 0.0                                                    # tau = 0
        if k % 5 == 3:
            row[:] = 0.0                                                     # no contact at all
        q = np.array([1.0, 0.0, 0.0, 0.0]) if k % 7 == 0 else _unit(rng)
        out.append((K, (rng.normal(size=3), q, rng.normal(size=3), L), row))
    return out


def test_query_against_restatement(pkg):
    """every field of admm_hip_rigid_query's record equals the plain Python restatement of rigid.hpp's order, bit for bit: random
    states and loads over spheres, boxes and meshes, general and diagonal anisotropic inertia, omega = 0, tau = 0, no load, q = 1"""
    rng = np.random.default_rng(7)
    for K, (c, q, v, L), row in _cases(rng, 60):
        S = _state(pkg, c, q, v, L, entry=3)
        for dt in (0.02, 1.0 / 60.0):
            got = pkg.rigid_query(S, row, dt, count=5, body=K)
            want = _restate(K, S, row, dt)
            for n in pkg.RIGID_FIELDS:
                assert np.asarray(getattr(got, n)).ravel().tobytes() == np.array(want[n], dtype=np.float64).tobytes(), (n, K["type"])
            assert got.count == 5 and got.entry == 3
    with pytest.raises(pkg.AdmmHipError):
        pkg.rigid_query(S, row, 0.0, body=K)
    with pytest.raises(pkg.AdmmHipError):
        pkg.rigid_query(S, row, 0.02, body=dict(K, inertia=[1.0, 0.0, 0.0, -1.0, 0.0, 1.0]))
    with pytest.raises(pkg.AdmmHipError):
        pkg.rigid_query(S, row, 0.02, body=dict(K, mass=0.0))


def test_query_against_long_double(pkg):
    """Stage by stage against long double, each stage taking the record's own doubles of the stage before as its input (as the rule
    does), u = 2^-53, gamma(k) = k u / (1 - k u).  A result that a leaf reaches through at most k rounded operations lies within
    gamma(k) times the sum of the magnitudes of its terms (negation and the factors 2 and dt / 2 are exact):
      v' = v + dt (F / m + a)          F passes /, +, *, +: gamma(4) (|v| + dt (|F| / m + |a|))
      L' = L + dt tau                  gamma(2) (|L| + dt |tau|)
      c' = c + dt v'                   gamma(2) (|c| + dt |v'|)
      R(q)                             a product, a sum, the subtraction from one (or a product, a sum): gamma(3) (1 + 2 (..)) with absolute values
      omega' = R (Jinv (R^T L'))       three products-and-sums of depth 3 each: gamma(9) |R| |Jinv| |R^T| |L'|; Jinv is the constant of the rule
                                       (the host's inverse, restated and checked bitwise in test_query_against_restatement)
      p = d (x) q                      h = (dt / 2) omega' rounds once; n2 = sum h^2 has positive terms, relative error gamma(5); 1 + n2 gamma(6);
                                       the root halves it and rounds: gamma(4); d_w = 1 / s gamma(5), d_xyz = h / s gamma(6); a product with q
                                       one more, at most three additions: |p_i - exact| <= e_i = gamma(10) sum_k |d_k| |q_k'|
      q' = p / |p|                     |p| from the computed p: gamma(3); the division one more; an error e of p moves p / |p| by at most
                                       (e_i + |q'_i| |e|_2) / |p| to first order: bound_i = (e_i + |q'_i| |e|_2) / |p| + gamma(4) |q'_i|
      par' = par0 + (c' - c0)          gamma(2) (|par0| + |c'| + |c0|)
    The long-double evaluation's own error (2^-64 per operation) is below u / 1000 of the same magnitudes; one more u in every gamma covers it."""
    rng = np.random.default_rng(11)
    worst = {}

    def check(name, got, ref, bound):
        err = np.abs(np.asarray(got, LD) - ref)
        ok = bound > 0
        if ok.any():
            worst[name] = max(worst.get(name, 0.0), float((err[ok] / bound[ok]).max()))
        assert np.all(err <= bound), (name, err, bound)

    for K, (c, q, v, L), row in _cases(rng, 60):
        dt = 0.02
        S = _state(pkg, c, q, v, L)
        O = pkg.rigid_query(S, row, dt, body=K)
        l = lambda a: np.asarray(a, LD)
        F, tau, m, a = -l(row[:3]), -l(row[3:]), LD(K["mass"]), l(K["accel"])
        check("v", O.v, l(v) + LD(dt) * (F / m + a), gamma(5) * (np.abs(l(v)) + LD(dt) * (np.abs(F) / m + np.abs(a))))
        check("L", O.L, l(L) + LD(dt) * tau, gamma(3) * (np.abs(l(L)) + LD(dt) * np.abs(tau)))
        check("c", O.c, l(c) + LD(dt) * l(O.v), gamma(3) * (np.abs(l(c)) + LD(dt) * np.abs(l(O.v))))

        def rot(qq):
            w, x, y, z = l(qq)
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], LD)
            w, x, y, z = np.abs(l(qq))
            M = np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x)],
                          [2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y)]], LD)
            return R, M
        R1, M1 = rot(O.q)
        check("R", O.R, R1, gamma(4) * M1)
        Rd = np.array(_rotation(S.q)).reshape(3, 3)                          # the rotation before the turn, as the rule rounds it
        Ji = _invert(K["inertia"])
        Jm = l([[Ji[0], Ji[1], Ji[2]], [Ji[1], Ji[3], Ji[4]], [Ji[2], Ji[4], Ji[5]]])
        check("omega", O.omega, l(Rd) @ (Jm @ (l(Rd).T @ l(O.L))), gamma(10) * (np.abs(l(Rd)) @ (np.abs(Jm) @ (np.abs(l(Rd)).T @ np.abs(l(O.L))))))
        h = LD(dt) / 2 * l(O.omega)
        s = np.sqrt(1 + h @ h)
        d = np.concatenate([[1 / s], h / s])
        qq = l(q)
        p = np.array([d[0] * qq[0] - (d[1] * qq[1] + d[2] * qq[2] + d[3] * qq[3]),
                      d[0] * qq[1] + d[1] * qq[0] + d[2] * qq[3] - d[3] * qq[2],
                      d[0] * qq[2] + d[2] * qq[0] + d[3] * qq[1] - d[1] * qq[3],
                      d[0] * qq[3] + d[3] * qq[0] + d[1] * qq[2] - d[2] * qq[1]], LD)
        mag = np.array([np.abs(d) @ np.abs(qq[[0, 1, 2, 3]]), np.abs(d) @ np.abs(qq[[1, 0, 3, 2]]), np.abs(d) @ np.abs(qq[[2, 3, 0, 1]]), np.abs(d) @ np.abs(qq[[3, 2, 1, 0]])], LD)
        e = gamma(11) * mag
        pn = np.sqrt(p @ p)
        qe = p / pn
        check("q", O.q, qe, (e + np.abs(qe) * np.sqrt(e @ e)) / pn + gamma(5) * np.abs(qe))
        if K["type"] == BOX:
            assert O.par.tobytes() == np.asarray(K["par0"], np.float64).tobytes()
        else:
            ref = l(K["par0"][:3]) + (l(O.c) - l(K["c0"]))
            check("par", O.par[:3], ref, gamma(3) * (np.abs(l(K["par0"][:3])) + np.abs(l(O.c)) + np.abs(l(K["c0"]))))
            assert O.par[3] == K["par0"][3]
    print("rigid_query against long double, largest error / bound per stage: %s" % {k: "%.3g" % v for k, v in worst.items()})


def test_rotation_quality_over_1000_torque_free_frames(pkg):
    """anisotropic J, L off every principal axis, no load: after 1000 frames |q| - 1 is within 4 ulp of one (normalise divides by the
    root of the computed |p|^2: gamma(4) to first order), R passes admm_frame::check -- the project's own 1e-12 criterion, asked of
    set_collision_frames in a host-only context -- and L has the bits it started with.  Every frame's rotation angle 2 atan2(|vec r|,
    r_w) of r = q' (x) conj(q), in long double, is within (dt |omega'|)^3 / 12 of dt |omega'| plus rounding: q and q' are unit to
    4 ulp and q' carries at most gamma(11) + gamma(5) per component (test_query_against_long_double), which moves the angle by at most
    twice the 2-norm of those: 2 * 2 * 16 u = 64 u."""
    K = dict(type=BOX, mass=2.0, inertia=[0.02, 0.0, 0.0, 0.05, 0.0, 0.11], accel=[0.0, 0.0, 0.0], c0=[0.0, 0.0, 0.0], par0=[0.1, 0.2, 0.3, 0.0])
    L0 = np.array([0.3, -0.2, 0.25])
    S = _state(pkg, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], L0)
    dt = 0.02
    worst_angle, worst_norm = 0.0, 0.0
    for f in range(1000):
        O = pkg.rigid_query(S, np.zeros(6), dt, body=K)
        q0, q1 = np.asarray(S.q, LD), np.asarray(O.q, LD)
        r = np.array([q1[0] * q0[0] + q1[1:] @ q0[1:], *(-q1[0] * q0[1:] + q0[0] * q1[1:] - np.cross(q1[1:], q0[1:]))], LD)
        angle = 2 * np.arctan2(np.sqrt(r[1:] @ r[1:]), np.abs(r[0]))
        w = LD(dt) * np.sqrt(np.asarray(O.omega, LD) @ np.asarray(O.omega, LD))
        assert abs(angle - w) <= w ** 3 / 12 + 64 * U, (f, float(angle - w), float(w ** 3 / 12))
        worst_angle = max(worst_angle, float(abs(angle - w) / (w ** 3 / 12)))
        worst_norm = max(worst_norm, float(abs(np.sqrt(q1 @ q1) - 1)))
        assert abs(np.sqrt(q1 @ q1) - 1) <= 4 * 2.0 ** -52
        assert O.L.tobytes() == L0.tobytes()
        S = O
    print("1000 torque-free frames: largest | |q| - 1 | = %.3g, largest angle defect / (w^3 / 12) = %.3g, dt |omega| = %.3g" % (worst_norm, worst_angle, float(w)))
    assert not np.array_equal(S.R, np.eye(3))
    h = pkg.System(device_id=-1)
    h.set_collision_shapes([SPHERE], [[0.0, 0.0, 0.0, 1.0]])
    h.set_collision_frames([np.concatenate([S.R.ravel(), S.c])])          # refused unless admm_frame::check(R) == 0


def test_free_fall(pkg):
    """K frames without a load: v has the bits of the loop v <- v + dt ((-0.0) / m + a), c those of c <- c + dt v, and c lies within a
    rounding bound of c0 + dt^2 a K (K + 1) / 2 (v0 = 0).  Bound: v_k = k (dt a) up to one rounding of dt a and k - 1 additions:
    |v_k - k dt a| <= gamma(k) k |dt a|; c_K = c0 + sum_k dt v_k, a product and an addition per frame:
    |c_K - exact| <= gamma(2 K + 1) (|c0| + dt^2 |a| K (K + 1) / 2)."""
    Kf, dt = 200, 0.02
    a = np.array([0.3, -9.8, 0.0])
    K = dict(type=SPHERE, mass=1.7, inertia=[0.01, 0.0, 0.0, 0.01, 0.0, 0.01], accel=a, c0=[0.5, 2.0, -1.0], par0=[0.5, 2.0, -1.0, 0.1])
    S = _state(pkg, K["c0"], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    v = [0.0, 0.0, 0.0]; c = [float(x) for x in K["c0"]]
    for f in range(Kf):
        S = pkg.rigid_query(S, np.zeros(6), dt, body=K)
        v = [v[j] + dt * ((-0.0) / K["mass"] + float(a[j])) for j in range(3)]
        c = [c[j] + dt * v[j] for j in range(3)]
        assert S.v.tobytes() == np.array(v).tobytes() and S.c.tobytes() == np.array(c).tobytes(), f
        assert S.q.tobytes() == np.array([1.0, 0.0, 0.0, 0.0]).tobytes() and not S.L.any() and not S.omega.any()
    tri = LD(Kf) * (Kf + 1) / 2
    exact = np.asarray(K["c0"], LD) + LD(dt) * LD(dt) * np.asarray(a, LD) * tri
    bound = gamma(2 * Kf + 1) * (np.abs(np.asarray(K["c0"], LD)) + LD(dt) * LD(dt) * np.abs(np.asarray(a, LD)) * tri)
    err = np.abs(np.asarray(S.c, LD) - exact)
    print("free fall, %d frames: error / bound %s" % (Kf, (err[bound > 0] / bound[bound > 0]).astype(float)))
    assert np.all(err <= bound)
    assert S.par[:3].tobytes() == np.array([K["par0"][j] + (c[j] - K["c0"][j]) for j in range(3)]).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
J1 = [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]
YAW = 0.3
RYAW = [math.cos(YAW), 0.0, math.sin(YAW), 0.0, 1.0, 0.0, -math.sin(YAW), 0.0, math.cos(YAW)]
EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def _host_scene(pkg, world=1):
    scene = _two_bars(pkg)
    s = _with_bodies(pkg, scene, device_id=-1, world=world)
    ia, ib = s.bodies
    ob = s.add_collision_mesh(*_cube(0.1, np.array([2.0, 0.0, 0.0])))
    s.types = [FLOOR, MESH, MESH, SPHERE, CYLINDER, BOX, MESH, SPHERE]
    s.params = [[0, -0.3, 0, 0], [0, 0, 0, ia], [0, 0, 0, ib], [1.0, 1.0, 1.0, 0.1], [0.0, 3.0, 0.0, 0.1], [0.1, 0.1, 0.1, 0.0], [0, 0, 0, ob], [3.0, 1.0, 1.0, 0.1]]
    s.set_collision_shapes(s.types, s.params)
    fr = [EYE + [0.0, 0.0, 0.0] for _ in s.types]
    fr[5] = EYE + [0.5, 0.5, 0.5]                                           # the box's centre
    fr[7] = RYAW + [3.0, 1.0, 1.0]                                          # a turned sphere, pivoted at its centre
    s.set_collision_frames(fr)
    return s


def test_refusals_and_order_of_checks(pkg):
    s = _host_scene(pkg)
    nan = float("nan")
    good = (1.0, J1, [1.0, 1.0, 1.0])
    # ADMM_ERR_ARG, in this order, each shown with arguments that a later check would refuse too (attribution is off throughout):
    for e in (-1, 8, 64):                                                  # the entry
        _refused(pkg, s, ADMM_ERR_ARG, ["entry %d" % e, "not an entry"], s.add_rigid_body, e, nan, J1, [0, 0, 0])
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 0", "floor", "infinite"], s.add_rigid_body, 0, nan, J1, [0, 0, 0])      # infinite shapes
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 4", "cylinder", "infinite"], s.add_rigid_body, 4, nan, J1, [0, 0, 0])
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 1", "surface"], s.add_rigid_body, 1, nan, J1, [0, 0, 0])                 # a surface of simulated nodes
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 2", "surface"], s.add_rigid_body, 2, 1.0, [nan] * 6, [0, 0, 0])
    for m in (nan, float("inf"), 0.0, -1.0):                               # mass and inertia
        _refused(pkg, s, ADMM_ERR_ARG, ["entry 3", "mass"], s.add_rigid_body, 3, m, J1, [1.0, 1.0, 1.0])
    for J in ([nan, 0, 0, 1, 0, 1], [1, 0, 0, float("inf"), 0, 1], [1, 0, 0, -1, 0, 1], [1, 2, 0, 1, 0, 1], [0, 0, 0, 1, 0, 1], [1, 0, 0, 1, 0, 0]):
        _refused(pkg, s, ADMM_ERR_ARG, ["entry 3", "inertia"], s.add_rigid_body, 3, 1.0, J, [1.0, 1.0, 1.0])
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 3", "not finite"], s.add_rigid_body, 3, 1.0, J1, [nan, 1.0, 1.0])
    # ADMM_ERR_STATE: contact attribution is off -- before the frame is looked at (entry 7's pivot is not this centre of mass)
    _refused(pkg, s, ADMM_ERR_STATE, ["entry 3", "attribution"], s.add_rigid_body, 3, *good)
    _refused(pkg, s, ADMM_ERR_STATE, ["entry 7", "attribution"], s.add_rigid_body, 7, 1.0, J1, [0.0, 0.0, 0.0])
    s.enable_contact_attribution(True)
    # ADMM_ERR_ARG: the frame -- a turned entry pivots at the centre of mass, a box's centre of mass is its pivot
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 7", "pivot"], s.add_rigid_body, 7, 1.0, J1, [3.0, 1.0, 1.5])
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 5", "box"], s.add_rigid_body, 5, 1.0, J1, [0.5, 0.5, 0.6])
    assert s.rigid_state() == []
    b0 = s.add_rigid_body(3, 1.0, J1, [1.0, 1.0, 1.2], accel=[0.0, -9.8, 0.0])      # the identity: any centre of mass
    b1 = s.add_rigid_body(7, 2.0, J1, [3.0, 1.0, 1.0])
    b2 = s.add_rigid_body(5, 1.0, J1, [0.5, 0.5, 0.5])
    b3 = s.add_rigid_body(6, 1.0, J1, [2.05, 0.05, 0.05])
    assert (b0, b1, b2, b3) == (0, 1, 2, 3)
    _refused(pkg, s, ADMM_ERR_ARG, ["entry 3", "already"], s.add_rigid_body, 3, *good)
    st = s.rigid_state()
    assert [r.entry for r in st] == [3, 7, 5, 6] and st[0].c.tolist() == [1.0, 1.0, 1.2] and st[0].q.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert np.abs(st[1].R.ravel() - np.array(RYAW)).max() < 4 * U and st[1].par.tolist() == [3.0, 1.0, 1.0, 0.1]
    assert st[0].body["accel"].tolist() == [0.0, -9.8, 0.0] and st[0].body["par0"].tolist() == [1.0, 1.0, 1.0, 0.1] and st[0].body["type"] == SPHERE
    # while a body exists: the switch stays on, the context stays unsharded, the list keeps its length and the bodies' types
    _refused(pkg, s, ADMM_ERR_STATE, ["entry 3", "rigid body"], s.enable_contact_attribution, False)
    _refused(pkg, s, ADMM_ERR_UNSUPPORTED, ["rigid body", "sharded"], s.set_shard, 0, 2)
    _refused(pkg, s, ADMM_ERR_STATE, ["rigid body", "length"], s.set_collision_shapes, s.types[:-1], s.params[:-1])
    ty = list(s.types); ty[3] = BOX
    _refused(pkg, s, ADMM_ERR_ARG, ["shape 3", "rigid body", "type"], s.set_collision_shapes, ty, s.params)
    moved = [list(p) for p in s.params]; moved[3][:3] = [9.0, 9.0, 9.0]
    s.set_collision_shapes(s.types, moved)                                 # the same length: taken, the body's params ignored
    # the state, the acceleration, the depth
    s.set_rigid_state(0, [0.0, 1.0, 0.0], [2.0, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 0.01])
    r = s.rigid_state()[0]
    assert r.q.tolist() == [1.0, 0.0, 0.0, 0.0] and r.par.tolist() == [1.0 + (0.0 - 1.0), 1.0 + (1.0 - 1.0), 1.0 + (0.0 - 1.2), 0.1]
    assert r.omega.tolist() == _omega(EYE, _invert(J1), [0.0, 0.0, 0.01]) and abs(r.omega[2] - 1.0) < 4 * U
    q = r.q.copy(); q[1] = 1e-9
    s.set_rigid_state(0, r.c, q, r.v, r.L)                                 # |q|^2 within 8 ulp of one: kept as given
    assert s.rigid_state()[0].q.tobytes() == q.tobytes()
    for bad in ([nan, 0, 0], [float("inf"), 0, 0]):
        _refused(pkg, s, ADMM_ERR_ARG, ["body 0", "entry 3", "not finite"], s.set_rigid_state, 0, bad, [1, 0, 0, 0], [0, 0, 0], [0, 0, 0])
        _refused(pkg, s, ADMM_ERR_ARG, ["body 0", "not finite"], s.set_rigid_state, 0, [0, 0, 0], [1, 0, 0, 0], [0, 0, 0], bad)
        _refused(pkg, s, ADMM_ERR_ARG, ["body 0", "not finite"], s.set_rigid_accel, 0, bad)
    _refused(pkg, s, ADMM_ERR_ARG, ["quaternion"], s.set_rigid_state, 0, [0, 0, 0], [0, 0, 0, 0], [0, 0, 0], [0, 0, 0])
    _refused(pkg, s, ADMM_ERR_ARG, ["quaternion"], s.set_rigid_state, 0, [0, 0, 0], [nan, 0, 0, 0], [0, 0, 0], [0, 0, 0])
    _refused(pkg, s, ADMM_ERR_ARG, ["body 4"], s.set_rigid_state, 4, [0, 0, 0], [1, 0, 0, 0], [0, 0, 0], [0, 0, 0])
    _refused(pkg, s, ADMM_ERR_ARG, ["body -1"], s.set_rigid_accel, -1, [0, 0, 0])
    s.set_rigid_accel(0, [0.0, -1.0, 0.0])
    assert s.rigid_body(0)["accel"].tolist() == [0.0, -1.0, 0.0]
    for bad in (-1e-9, nan):
        _refused(pkg, s, ADMM_ERR_ARG, ["depth_min"], s.set_rigid_depth, bad)
    s.set_rigid_depth(1e-9)
    s.initialize()                                                         # a host-only context finalizes with bodies

    # a sharded context: ARG before STATE before UNSUPPORTED
    t = _host_scene(pkg, world=2)
    _refused(pkg, t, ADMM_ERR_ARG, ["mass"], t.add_rigid_body, 3, nan, J1, [1.0, 1.0, 1.0])
    _refused(pkg, t, ADMM_ERR_STATE, ["attribution"], t.add_rigid_body, 3, *good)
    t.enable_contact_attribution(True)
    _refused(pkg, t, ADMM_ERR_UNSUPPORTED, ["entry 3", "sharded"], t.add_rigid_body, 3, *good)
    _refused(pkg, t, ADMM_ERR_UNSUPPORTED, ["entry 7", "sharded"], t.add_rigid_body, 7, 1.0, J1, [0.0, 0.0, 0.0])      # ... before the frame


def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    compile_cpp("rigid", pkg)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: scenes
# ---------------------------------------------------------------------------------------------------------------------------------
G = [0.0, -9.8, 0.0]
BALL_R, BALL_M = 0.06, 2.0
BALL_C = [0.07, 0.15 + BALL_R + 0.004, 0.15]
BALL_J = [0.4 * BALL_M * BALL_R ** 2 * d for d in (1, 0, 0, 1, 0, 1)]


def _ball_on_bars(pkg, body=True, setup=None, attribution=True):
    """scene 1: the two-bar drop of test_body_collision (both surfaces and a floor in the list) and a sphere of 2 kg, 4 mm above the
    top of bar A (13.5 kg), as the list's last entry; `body`: it is a rigid body under gravity, else it stays where it is"""
    scene = _two_bars(pkg)
    s = _with_bodies(pkg, scene)
    ia, ib = s.bodies
    s.types = [FLOOR, MESH, MESH, SPHERE]
    s.params = [[0, -0.3, 0, 0], [0, 0, 0, ia], [0, 0, 0, ib], BALL_C + [BALL_R]]
    s.set_collision_shapes(s.types, s.params)
    s.n_tet_batches = 3
    if setup:
        setup(s)
    if attribution:
        s.enable_contact_attribution(True)
    if body:
        s.add_rigid_body(3, BALL_M, BALL_J, BALL_C, G)
    return s


def _box_on_patch(pkg, body=True):
    """scene 2: a 9 x 9 patch of cloth nodes 5 cm apart in the plane y = 0, corners anchored, a collision element on every node; a box
    of half extents (0.25, 0.05, 0.25), 5 kg, turned by 0.3 rad about y, its bottom face 5 mm below the patch and its centre 3 cm and
    2 cm off the patch's: all 81 nodes are in contact with it, more than one 64-contact block in its row.  Friction 0.5; the box starts
    with a velocity along and into the patch."""
    n = 9
    g = np.linspace(-0.2, 0.2, n)
    xs = np.array([[g[i], 0.0, g[j]] for j in range(n) for i in range(n)])
    tris = []
    for j in range(n - 1):
        for i in range(n - 1):
            p = i + n * j
            tris += [(p, p + n, p + 1), (p + 1, p + n, p + n + 1)]
    tris = np.array(tris, np.int32)
    corners = np.array([0, n - 1, n * (n - 1), n * n - 1], np.int32)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(xs.ravel(), np.full(3 * len(xs), 0.025))
    s.add_forces(KIND["TRI_STRAIN"], tris, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["ANCHOR"], corners, [1000.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(xs), dtype=np.int32), [32.0])
    c = [0.03, 0.045, 0.02]
    s.types, s.params = [BOX], [[0.25, 0.05, 0.25, 0.0]]
    s.set_collision_shapes(s.types, s.params)
    s.set_collision_frames([RYAW + c])
    s.set_collision_friction([0.5])
    s.enable_contact_attribution(True)
    s.n_tet_batches = 3
    if body:
        m, h = 5.0, (0.25, 0.05, 0.25)
        J = [m / 3.0 * (h[1] ** 2 + h[2] ** 2), 0.0, 0.0, m / 3.0 * (h[0] ** 2 + h[2] ** 2), 0.0, m / 3.0 * (h[0] ** 2 + h[1] ** 2)]
        b = s.add_rigid_body(0, m, J, c, G)
        r = s.rigid_state()[b]
        s.set_rigid_state(b, r.c, r.q, [0.15, -0.1, 0.05], [0.0, 0.02, 0.0])
    return s


CUBE_H, CUBE_AT = 0.08, np.array([0.03, 0.153, 0.12])


def _cube_on_bars(pkg, body=True):
    """scene 3: the two bars under the list [static floor, body, static sphere, body].  Entry 3 is a closed obstacle mesh, a cube of 12
    triangles and 8 cm, 3 mm above bar A and off its axis (registered first: body 0); entry 1 is a sphere far from everything (body 1:
    its row stays empty); the floor touches bar A's underside (2 mm) and the static sphere presses into A's free end, so the empty row
    lies between rows with contacts."""
    scene = _two_bars(pkg)
    s = _with_bodies(pkg, scene)
    ob = s.add_collision_mesh(*_cube(CUBE_H, CUBE_AT))
    s.types = [FLOOR, SPHERE, SPHERE, MESH]
    s.params = [[0, 0.002, 0, 0], [5.0, 5.0, 5.0, 0.1], [0.05, 0.185, 0.55, 0.05], [0, 0, 0, ob]]
    s.set_collision_shapes(s.types, s.params)
    s.enable_contact_attribution(True)
    s.n_tet_batches = 3
    if body:
        m = 1.5
        s.add_rigid_body(3, m, [m * CUBE_H ** 2 / 6.0 * d for d in (1, 0, 0, 1, 0, 1)], CUBE_AT + CUBE_H / 2, G)
        s.add_rigid_body(1, 1.0, J1, [5.0, 5.0, 5.0], [0.0, -1.0, 0.0])
    return s


def _move_from_outside(b, states, n_entries):
    """the setters that exist without the feature, with the pose fields rigid_state returns"""
    par = [list(p) for p in b.params]
    fr = np.array(b.frames0, float).reshape(n_entries, 12).copy()
    mo = np.zeros((n_entries, 9))
    for r in states:
        par[r.entry] = r.par.tolist(); fr[r.entry] = r.frame; mo[r.entry] = r.motion
    b.set_collision_shapes(b.types, par)
    b.set_collision_frames(fr)
    b.set_collision_motion(mo)


def _device_against_outside(pkg, make, frames, iters=10, depth_min=DEPTH):
    """context A with the bodies on the device; every frame its new records must be rigid_query of the old ones and the rows of
    entry_resultants about the old centres, in every field; context B (make(body=False)) has no body and is moved by the setters
    before every step: x and v of the two must be the same bits.  -> per frame (x, v, states, counts) of A"""
    a, b = make(True), make(False)
    a.initialize(); b.initialize()
    a.set_rigid_depth(depth_min)
    ne = len(a.types)
    b.frames0 = getattr(b, "frames0", None) or [EYE + [0.0, 0.0, 0.0]] * ne
    out = []
    for f in range(frames):
        S = a.rigid_state()
        _move_from_outside(b, S, ne)
        a.step(iters); b.step(iters)
        new = a.rigid_state()
        cnts = None
        for k, r in enumerate(S):
            F, T, cnt = a.entry_resultants(pivot=r.c, depth_min=depth_min)
            want = pkg.rigid_query(r, np.concatenate([F[r.entry], T[r.entry]]), DT, count=int(cnt[r.entry]))
            for n in pkg.RIGID_FIELDS:
                assert getattr(want, n).tobytes() == getattr(new[k], n).tobytes(), (f, k, n, getattr(want, n), getattr(new[k], n))
            assert want.count == new[k].count and new[k].entry == r.entry, (f, k)
            assert new[k].F.tobytes() == (-F[r.entry]).tobytes() and new[k].tau.tobytes() == (-T[r.entry]).tobytes()
            cnts = cnt
        xa, va = a.m_x.copy(), a.m_v.copy()
        assert xa.tobytes() == b.m_x.tobytes(), (f, "x", np.abs(xa - b.m_x).max())
        assert va.tobytes() == b.m_v.tobytes(), (f, "v")
        assert np.isfinite(xa).all()
        out.append((xa, va, new, cnts))
    return out, a


@pytest.mark.gpu
def test_ball_on_bars_device_against_the_rule_from_outside(pkg):
    res, a = _device_against_outside(pkg, lambda body: _ball_on_bars(pkg, body), 8)
    counts = [r[2][0].count for r in res]
    print("ball on bars: contacts of the body per frame %s, F_y %s, centre y %.4f -> %.4f" % (counts, ["%.3g" % r[2][0].F[1] for r in res], BALL_C[1], res[-1][2][0].c[1]))
    assert max(counts) > 0 and counts[0] == 0                              # free fall first, then contact
    assert any(r[2][0].F[1] > 0.0 for r in res)                            # the bar pushes the ball up


@pytest.mark.gpu
def test_box_on_patch_device_against_the_rule_from_outside(pkg):
    def make(body):
        s = _box_on_patch(pkg, body)
        s.frames0 = [RYAW + [0.03, 0.045, 0.02]]
        return s
    res, a = _device_against_outside(pkg, make, 8)
    counts = [r[2][0].count for r in res]
    print("box on patch: contacts per frame %s, |tau| %s, framed R01 %.3g" % (counts, ["%.3g" % np.abs(r[2][0].tau).max() for r in res], res[-1][2][0].R[0, 2]))
    assert max(counts) > 64                                                # the row crosses a 64-contact block
    assert any(np.abs(r[2][0].tau).max() > 0.0 for r in res)              # pressed off-centre
    assert any(np.abs(r[2][0].F[[0, 2]]).max() > 0.0 for r in res)        # friction: a tangential load


@pytest.mark.gpu
def test_cube_on_bars_device_against_the_rule_from_outside(pkg):
    res, a = _device_against_outside(pkg, lambda body: _cube_on_bars(pkg, body), 8)
    cube = [r[2][0].count for r in res]; far = [r[2][1].count for r in res]
    rows = [r[3].tolist() for r in res]
    print("cube on bars: contacts of the cube per frame %s, of the far body %s, rows of the last frame %s; omega %s" % (cube, far, rows[-1], res[-1][2][0].omega))
    assert max(cube) > 0 and max(far) == 0
    assert any(c[0] > 0 and c[1] == 0 and c[2] > 0 and c[3] > 0 for c in rows)      # an empty body row between rows with contacts
    assert np.abs(res[-1][2][0].omega).max() > 0.0                         # off its axis: it turns, and the mesh entry is framed
    v = [0.0, 0.0, 0.0]                                                    # the far body is bitwise in free fall
    for f, r in enumerate(res):
        v = [v[j] + DT * ((-0.0) / 1.0 + [0.0, -1.0, 0.0][j]) for j in range(3)]
        assert r[2][1].v.tobytes() == np.array(v).tobytes(), f


def _frames(s, frames, iters=10, start=0):
    out = []
    for f in range(frames):
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


def _same_frames(p, q):
    return len(p) == len(q) and all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(p, q))


@pytest.mark.gpu
def test_a_stale_upload_of_the_shape_table_is_healed(pkg):
    """after 3 frames set_collision_friction with the coefficients in effect and set_collision_shapes with the list as first given
    upload the host's table, whose rows for the body are those of the registration; the next step's pose launch writes the body's
    rows again, so the frames equal those of a context that made no such call"""
    a, b = _ball_on_bars(pkg), _ball_on_bars(pkg)
    a.initialize(); b.initialize()
    fa, fb = _frames(a, 3), _frames(b, 3)
    a.set_collision_friction([0.0] * 4)
    a.set_collision_shapes(a.types, a.params)
    counts = []
    for f in range(6):
        fa += _frames(a, 1); fb += _frames(b, 1)
        counts.append(b.rigid_state()[0].count)                            # (read from b: a's host table stays stale until the end)
    assert _same_frames(fa, fb)
    ra, rb = a.rigid_state()[0], b.rigid_state()[0]
    assert ra.same_bits(rb) and max(counts) > 0 and ra.c[1] < BALL_C[1] - 0.004


@pytest.mark.gpu
def test_launch_modes_give_the_same_frames(pkg, monkeypatch):
    """scene 1 with ADMM_HIP_GRAPH = 0 (the eager loop), = 1, ADMM_HIP_FRAME_GRAPH = 0 and the default: the same x, v and records"""
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = _ball_on_bars(pkg)
        s.initialize()
        fr = _frames(s, 8)
        g = s.graph_state()
        assert bool(g["iter_graph"]) == (env.get("ADMM_HIP_GRAPH") != "0")
        res[tuple(env.items())] = (fr, s.rigid_state()[0])
    keys = list(res)
    assert res[keys[0]][1].count > 0
    for k in keys[1:]:
        assert _same_frames(res[keys[0]][0], res[k][0]) and res[keys[0]][1].same_bits(res[k][1]), k


def _opt_tolerance(s):
    s.set_tolerance(2e-3, 2e-3, 2)


def _opt_anderson(s):
    s.set_acceleration(2)


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["tolerance", "anderson", "surface_reaction"])
def test_options_device_against_the_rule_from_outside(pkg, option):
    """an exit by tolerance, Anderson acceleration with window 2, and a surface-reaction share on bar A's surface in the same scene: these
    change the frames themselves, so each is held to the rule applied from outside and to its twin under the same option (both run
    the eager loop), as the graph modes above are held to the eager default"""
    setup = dict(tolerance=_opt_tolerance, anderson=_opt_anderson).get(option)

    def make(body):
        s = _ball_on_bars(pkg, body, setup=setup)
        if option == "surface_reaction":
            s.set_surface_reaction(s.bodies[0], 0.5)
        return s
    res, a = _device_against_outside(pkg, make, 8, iters=20 if option == "tolerance" else 10)
    assert max(r[2][0].count for r in res) > 0
    if option == "surface_reaction":
        assert a.surface_reaction()[2]["n_contacts"] > 0


@pytest.mark.gpu
def test_the_two_consumers_of_one_frame_keep_their_own_depths(pkg):
    """two-way contact and the rigid bodies run the same contact chain in one frame, each with its own depth_min: neither may read the
    other's compaction.  Scene 1 with a share of 0.5 on bar A's surface; six frames bring the ball and bar B onto bar A, then one frame
    (a) as it is, both depths 0, (b) with set_rigid_depth(d_r), (c) with set_surface_reaction_depth(d_s).  The runs are the same bits up
    to that frame, so d_r and d_s come from (a)'s contacts of that frame: the middle between the shallowest and the deepest contact of
    the ball, and of bar A's surface.  At least one contact lies between 0 and either depth (asserted through contacts(depth_min)
    counts), and each setting does change its own consumer (asserted).  (a) against (b): the surface report's dv and the nodes' v,
    bitwise.  (a) against (c): the body's record, bitwise."""
    def run(rigid_depth=None, surface_depth=None):
        s = _ball_on_bars(pkg, True)
        s.set_surface_reaction(s.bodies[0], 0.5)
        s.initialize()
        for _ in range(6):
            s.step(10)
        if rigid_depth is not None:
            s.set_rigid_depth(rigid_depth)
        if surface_depth is not None:
            s.set_surface_reaction_depth(surface_depth)
        s.step(10)
        return s

    def body(s):
        r = s.rigid_state()[0]
        return b"".join(getattr(r, n).tobytes() for n in pkg.RIGID_FIELDS), r.count

    a = run()
    c, o = a.contacts(depth_min=0.0), a.contact_owners(depth_min=0.0)
    assert np.array_equal(c["node"], o["node"])
    ball, surf = np.sort(c["depth"][o["entry"] == 3]), np.sort(c["depth"][o["entry"] == 1])
    assert len(ball) >= 2 and len(surf) >= 2 and ball[0] < ball[-1] and surf[0] < surf[-1], (ball, surf)
    d_r, d_s = 0.5 * (ball[0] + ball[-1]), 0.5 * (surf[0] + surf[-1])
    n0 = len(c)
    print("cross-talk: %d contacts, the ball's depths %s, the surface's %s, d_r %.3g (%d contacts above), d_s %.3g (%d above)" %
          (n0, ball, surf, d_r, len(a.contacts(depth_min=d_r)), d_s, len(a.contacts(depth_min=d_s))))
    assert len(a.contacts(depth_min=d_r)) < n0 and len(a.contacts(depth_min=d_s)) < n0      # a contact between 0 and either depth
    dv_a, _, info_a = a.surface_reaction()
    assert info_a["n_reacting"] >= 2 and body(a)[1] == len(ball)
    b = run(rigid_depth=d_r)
    dv_b, _, info_b = b.surface_reaction()
    assert dv_b.tobytes() == dv_a.tobytes() and info_b == info_a and b.m_v.tobytes() == a.m_v.tobytes() and b.m_x.tobytes() == a.m_x.tobytes()
    assert body(b)[1] < body(a)[1] and body(b)[0] != body(a)[0]          # the setting reached its own consumer
    k = run(surface_depth=d_s)
    assert body(k) == body(a)
    dv_k, _, info_k = k.surface_reaction()
    assert info_k["n_contacts"] < info_a["n_contacts"] and dv_k.tobytes() != dv_a.tobytes()      # the setting reached its own consumer


@pytest.mark.gpu
def test_off_is_off(pkg):
    """no body registered: the frames of the scene built without touching the new calls, bit for bit -- with attribution on and the
    feature's depth set and its (empty) state read, and against the plain scene with attribution off"""
    plain = _ball_on_bars(pkg, body=False, attribution=False); plain.initialize()
    never = _ball_on_bars(pkg, body=False); never.initialize()
    touched = _ball_on_bars(pkg, body=False); touched.set_rigid_depth(1e-9); touched.initialize(); touched.set_rigid_depth(0.0)
    assert touched.rigid_state() == []
    fp, fn, ft = _frames(plain, 10), _frames(never, 10), _frames(touched, 10)
    assert touched.rigid_state() == []
    assert _same_frames(fn, ft) and _same_frames(fp, fn)


@pytest.mark.gpu
def test_checkpoint(pkg):
    """4 frames; x, v, every batch's u and warm start and the body's c, q, v, L go into a fresh context; its next 4 frames are those
    of 8 frames straight"""
    a = _ball_on_bars(pkg); a.initialize()
    _frames(a, 4)
    X, V = a.m_x.copy(), a.m_v.copy()
    loc = [a.read_local(b) for b in range(3)]
    r = a.rigid_state()[0]
    assert r.count > 0
    rest = _frames(a, 4)
    b = _ball_on_bars(pkg); b.initialize()
    b.m_x = X; b.m_v = V
    for k, l in enumerate(loc):
        b.write_local(k, u=l["u"], state=l["state"] if l["state"].shape[1] == 4 else None)
    b.set_rigid_state(0, r.c, r.q, r.v, r.L)
    got = _frames(b, 4)
    assert _same_frames(rest, got)
    ra, rb = a.rigid_state()[0], b.rigid_state()[0]
    assert ra.same_bits(rb)


def _ball_on_block(pkg, body):
    """a block of 4 x 3 x 4 cells of 5 cm (density 200: 1.2 kg), anchored at its base y = 0, no gravity, a collision element on every
    node; a sphere of the block's mass, radius 10 cm (the block's half width: as it sinks it meets the top's nodes one ring after the
    other, 5 at 1.3 cm, 9 at 2.9 cm), 1 cm above the centre of its top, under gravity when `body`"""
    mg = pkg.meshgen
    x, tets = mg.bar(4, 3, 4)
    m = mg.lumped_tet_mass(x, tets, 200.0)
    base = np.flatnonzero(x[:, 1] == 0.0).astype(np.int32)
    top = int(np.flatnonzero((np.abs(x[:, 0] - 0.1) < 1e-12) & (np.abs(x[:, 1] - 0.15) < 1e-12) & (np.abs(x[:, 2] - 0.1) < 1e-12))[0])
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets.astype(np.int32), [2e4])
    s.add_forces(KIND["ANCHOR"], base, [1000.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    rad = 0.1
    c = [0.1, 0.15 + rad + 0.01, 0.1]
    s.set_collision_shapes([SPHERE], [c + [rad]])
    s.enable_contact_attribution(True)
    M = float(m.sum())
    if body:
        s.add_rigid_body(0, M, [0.4 * M * rad ** 2 * d for d in (1, 0, 0, 1, 0, 1)], c, G)
    s.initialize()
    return s, x, top, M, c


@pytest.mark.gpu
def test_a_falling_sphere_is_caught_by_a_soft_block(pkg):
    """Signs and orderings only.  Until the first frame with a contact the sphere is bitwise in free fall; from that frame on its v_y is
    strictly above the free-fall value of the same frame; at the end its centre is above the block's base plane; the block's
    top-centre node is lower than at rest by more than 1000 times its displacement in the same scene with the sphere left kinematic
    (no contact there).  Printed, not asserted: the mean contact force over the last 10 frames over m g.
    Measured on the MI355X: first contact in frame 2; the top-centre node down by 5.3 mm at the end (23.5 mm at most) against 1.7e-16 m
    with the sphere kinematic; the sphere's centre ends at y = 0.2346; mean contact force over the last 10 frames 0.982 m g."""
    frames = 40
    on, x, top, M, c0 = _ball_on_block(pkg, True)
    off = _ball_on_block(pkg, False)[0]
    v = [0.0, 0.0, 0.0]; c = list(c0)
    first, d_off, lowest, fy = None, 0.0, 0.0, []
    for f in range(frames):
        on.step(10); off.step(10)
        r = on.rigid_state()[0]
        v = [v[j] + DT * ((-0.0) / M + G[j]) for j in range(3)]
        c = [c[j] + DT * v[j] for j in range(3)]
        if first is None and r.count > 0:
            first = f
        if first is None:
            assert r.v.tobytes() == np.array(v).tobytes() and r.c.tobytes() == np.array(c).tobytes(), f
        else:
            assert r.v[1] > v[1], (f, r.v[1], v[1])
        assert np.isfinite(on.m_x).all()
        d_off = max(d_off, float(abs(off.m_x.reshape(-1, 3)[top, 1] - x[top, 1])))
        lowest = max(lowest, float(x[top, 1] - on.m_x.reshape(-1, 3)[top, 1]))
        fy.append(r.F[1])
    down = float(x[top, 1] - on.m_x.reshape(-1, 3)[top, 1])
    ratio = float(np.mean(fy[-10:]) / (M * 9.8))
    print("sphere on block: first contact in frame %s; top-centre node down by %.4g m at the end (most %.4g m), %.3g m with the sphere kinematic; "
          "centre y %.4f; mean contact force over the last 10 frames / (m g) = %.3f" % (first, down, lowest, d_off, r.c[1], ratio))
    assert first is not None and first > 0
    assert r.c[1] > 0.0
    assert down > 1000.0 * d_off and down > 0.0


@pytest.mark.gpu
def test_class_api_reproduces_the_python_records(pkg, tmp_path):
    """tests/cpp/rigid.cpp: scene 1 through the class mirror (CollisionShape::rigid_mass / rigid_inertia / rigid_accel,
    Settings::contact_attribution, System::rigid_state) gives the record of the Python run after 4 frames, bit for bit"""
    import subprocess
    from test_cpp_host import compile_cpp
    exe = compile_cpp("rigid", pkg)
    scene = _two_bars(pkg)
    x, tets, anch, m, na, (sa, sb) = scene
    frames, iters = 4, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(tets), len(anch), na, len(sa), len(sb)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (tets, anch, sa, sb):
            a.astype(np.int32).tofile(f)
        np.array([-0.3, DT] + BALL_C + [BALL_R, BALL_M] + BALL_J + G).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s = _ball_on_bars(pkg); s.initialize()
    _frames(s, frames, iters)
    want = s.rigid_state()[0].record()
    assert want.count > 0
    assert open(outp, "rb").read() == bytes(want)
