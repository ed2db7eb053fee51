"""Rigid attachments: whole anchor batches fastened to rigid bodies (System.attach_anchors, admm_hip_attach_anchors; csrc/attach.hpp).

CPU (no GPU, host-only contexts): attachment_query bit for bit against a plain Python restatement of attach.hpp's order and against
long double within bounds derived from the operation counts; the sign bits of a row that takes no add; every refusal and the order of
the checks; the class mirror compiles.
GPU: the device bit for bit against the rule applied from outside on three scenes, together with a twin context without body and
attachment that is moved by the setters and update_anchors; a context without a collision batch; launch modes and solver options; off is
off; a checkpoint; attaching after finalize and detaching mid-run; the linear momentum's balance; the behaviour the feature exists for;
the class mirror."""

import numpy as np
import pytest

from checkers import KIND
from test_body_collision import _two_bars, _refused, DT, MESH, FLOOR
from test_reactions import _documented_sum
from test_rigid_bodies import gamma, U, LD, DEPTH, SPHERE, BOX, RYAW, EYE, J1, G, _unit, _rotation, _move_from_outside, _frames, _same_frames, _host_scene

ADMM_ERR_ARG, ADMM_ERR_HIP, ADMM_ERR_STATE, ADMM_ERR_UNSUPPORTED = 1, 2, 3, 4
COUNTS = (1, 63, 64, 65, 130, 257 * 64 + 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule, restated (csrc/attach.hpp's header comment, operation by operation, on Python floats)
# ---------------------------------------------------------------------------------------------------------------------------------
def _local_offset(c, R, t):
    c, R, t = [float(v) for v in c], [float(v) for v in np.ravel(R)], [float(v) for v in t]
    e = [t[j] - c[j] for j in range(3)]
    return [R[j] * e[0] + (R[3 + j] * e[1] + R[6 + j] * e[2]) for j in range(3)]


def _target(c, R, r):
    c, R, r = [float(v) for v in c], [float(v) for v in np.ravel(R)], [float(v) for v in r]
    return [c[j] + (R[3 * j] * r[0] + (R[3 * j + 1] * r[1] + R[3 * j + 2] * r[2])) for j in range(3)]


def _terms(f, p, pv):
    f, p, pv = [float(v) for v in f], [float(v) for v in p], [float(v) for v in pv]
    r = [p[j] - pv[j] for j in range(3)]
    return [f[0], f[1], f[2], r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]]


def _row(f, point, active, pivot):
    """six sums over ALL elements in index order, a released one adding six +0.0, each in reaction.hpp's two-stage order"""
    t = [_terms(f[i], point[i], pivot) if active[i] else [0.0] * 6 for i in range(len(f))]
    return np.array([_documented_sum([ti[q] for ti in t]) for q in range(6)])


def _pose(rng, k):
    q = np.array([1.0, 0.0, 0.0, 0.0]) if k % 3 == 0 else _unit(rng)
    return rng.normal(size=3) * 10.0 ** rng.integers(-1, 2), np.array(_rotation(q))


def _flags(rng, n, k):
    if k % 3 == 0:
        return np.ones(n, np.int32)
    a = (rng.uniform(size=n) < (0.5 if k % 3 == 1 else 0.9)).astype(np.int32)
    a[0] = 0
    return a


def test_query_against_restatement(pkg):
    """targets and sums of admm_hip_attachment_query equal the plain Python restatement, bit for bit: identity and general q; 1, 63,
    64, 65 and 130 elements (the 64-block's padding and the first-stage fold at their edges) and 257 * 64 + 3 (more than 256 first-stage
    partials: the second stage wraps); all active and mixes of released elements, the first one among them"""
    rng = np.random.default_rng(3)
    for k, n in enumerate(COUNTS * 2):
        c, R = _pose(rng, k)
        loc = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-2, 1)
        got = pkg.attachment_query(c=c, R=R, local=loc)["targets"]
        m = min(n, 200)                                                    # (the targets are elementwise: the large count adds nothing)
        want = np.array([_target(c, R, loc[i]) for i in range(m)])
        assert got[:m].tobytes() == want.tobytes(), n
        f = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-2, 3); p = rng.normal(size=(n, 3)); pv = rng.normal(size=3)
        act = _flags(rng, n, k)
        q = pkg.attachment_query(f=f, point=p, active=act, pivot=pv)
        assert q["row"].tobytes() == _row(f, p, act, pv).tobytes(), (n, k)
        assert q["n_active"] == int(act.sum())
        if k % 3 == 0:
            assert pkg.attachment_query(f=f, point=p, pivot=pv)["row"].tobytes() == q["row"].tobytes()      # active = None: all active
    # the offset's order (host only): what get_attachment reports for a derived offset is checked in the refusal test below


def test_query_against_long_double(pkg):
    """u = 2^-53, gamma(k) = k u / (1 - k u).  A result that a leaf reaches through at most k rounded operations lies within gamma(k)
    times the sum of the magnitudes of its terms.
      t_j = c_j + (R_j0 r_0 + (R_j1 r_1 + R_j2 r_2))     the deepest leaf passes a product and three additions: gamma(4) (|c_j| + sum_k |R_jk| |r_k|)
      a torque term r_a f_b - r_b f_a, r = p - pivot      a difference, a product, a difference: gamma(3) ((|p_a| + |pv_a|) |f_b| + (|p_b| + |pv_b|) |f_a|);
                                                          a force term is the input itself
      the sum of n terms                                  six additions of the block fold, ceil(nb / 256) - 1 rounded additions of a second-stage
                                                          lane (0.0 + p is exact) and eight of its fold: D = 6 + ceil(nb / 256) + 7 additions deep
    so a row's component lies within gamma(3 + D) sum_i mag_i of the exact sum.  The long-double evaluation's own error (2^-64 per
    operation) is below u / 1000 of the same magnitudes; one more u in every gamma covers it."""
    rng = np.random.default_rng(5)
    worst = {"targets": 0.0, "row": 0.0}
    for k, n in enumerate(COUNTS):
        c, R = _pose(rng, k + 1)
        loc = rng.normal(size=(n, 3))
        got = pkg.attachment_query(c=c, R=R, local=loc)["targets"]
        ref = np.asarray(c, LD) + np.asarray(loc, LD) @ np.asarray(R, LD).reshape(3, 3).T
        bound = gamma(5) * (np.abs(np.asarray(c, LD)) + np.abs(np.asarray(loc, LD)) @ np.abs(np.asarray(R, LD)).reshape(3, 3).T)
        err = np.abs(np.asarray(got, LD) - ref)
        assert np.all(err <= bound), n
        worst["targets"] = max(worst["targets"], float((err / bound).max()))
        f = rng.normal(size=(n, 3)) * 10.0; p = rng.normal(size=(n, 3)); pv = rng.normal(size=3)
        act = _flags(rng, n, k)
        q = pkg.attachment_query(f=f, point=p, active=act, pivot=pv)
        on = act != 0
        fl, rl = np.asarray(f, LD)[on], (np.asarray(p, LD) - np.asarray(pv, LD))[on]
        ref = np.concatenate([fl.sum(0), np.cross(rl, fl).sum(0)]) if on.any() else np.zeros(6, LD)
        fa, ra = np.abs(fl), (np.abs(np.asarray(p, LD)) + np.abs(np.asarray(pv, LD)))[on]
        mag = np.concatenate([fa.sum(0), np.array([(ra[:, 1] * fa[:, 2] + ra[:, 2] * fa[:, 1]).sum(), (ra[:, 2] * fa[:, 0] + ra[:, 0] * fa[:, 2]).sum(),
                                                   (ra[:, 0] * fa[:, 1] + ra[:, 1] * fa[:, 0]).sum()], LD)])
        nb = (n + 63) // 64
        D = 6 + (nb + 255) // 256 + 7
        bound = gamma(3 + D + 1) * mag
        err = np.abs(np.asarray(q["row"], LD) - ref)
        assert np.all(err <= bound), (n, err, bound)
        if on.any():
            worst["row"] = max(worst["row"], float((err / bound).max()))
    print("attachment_query against long double, largest error / bound: %s" % {k: "%.3g" % v for k, v in worst.items()})


def test_a_row_without_elements_is_plus_zero_and_is_not_added(pkg):
    """The sums of no element and of released elements only are six +0.0, sign bit clear -- and still a body without a batch must not
    take the add: -0.0 + 0.0 is +0.0, so adding such a row would clear the sign bit of a contact component that is -0.0, and the sign
    of the row is the sign of the record's F and tau (rigid_query: F = -Fe).  The device's side of it -- a body that carries nothing
    has F = -(its contact row), bit for bit -- is asserted in the two-body scene below."""
    zero = np.zeros(6).tobytes()
    assert pkg.attachment_query(f=np.zeros((0, 3)), point=np.zeros((0, 3)), pivot=[0.1, 0.2, 0.3])["row"].tobytes() == zero
    rng = np.random.default_rng(9)
    for n in (1, 64, 65):
        q = pkg.attachment_query(f=rng.normal(size=(n, 3)), point=rng.normal(size=(n, 3)), active=np.zeros(n, np.int32), pivot=rng.normal(size=3))
        assert q["row"].tobytes() == zero and q["n_active"] == 0
    neg = np.full(6, -0.0)
    assert np.signbit(neg).all() and not np.signbit(neg + np.zeros(6)).any()                 # what the add would do to a -0.0 row
    from test_rigid_bodies import _state
    K = dict(type=SPHERE, mass=2.0, inertia=J1, accel=[0.0, 0.0, 0.0], c0=[0.0, 0.0, 0.0], par0=[0.0, 0.0, 0.0, 0.1])
    S = _state(pkg, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    kept, added = pkg.rigid_query(S, neg, DT, body=K), pkg.rigid_query(S, neg + np.zeros(6), DT, body=K)
    assert not np.signbit(kept.F).any() and np.signbit(added.F).all()                        # the record shows which row it got


def test_refusals_and_order_of_checks(pkg):
    s = _host_scene(pkg)                                                   # batches: 0 tets, 1 anchors (static), 2 collision
    x = _two_bars(pkg)[0]
    free = np.array([40, 41, 42], np.int32)
    mv = s.add_forces(KIND["ANCHOR"], free, [1000.0, 1.0], targets=x[free] + 0.01)
    assert mv == 3
    nan, inf = float("nan"), float("inf")
    bad = np.full((3, 3), nan)
    s.enable_contact_attribution(True)
    # ADMM_ERR_ARG, in this order, each shown with arguments that a later check would refuse too (there is no body yet)
    for k in (-1, 0, 2, 4, 64):
        _refused(pkg, s, ADMM_ERR_ARG, ["batch %d" % k, "not an anchor batch"], s.attach_anchors, k, 7, None)
    _refused(pkg, s, ADMM_ERR_ARG, ["body 0", "not a rigid body"], s.attach_anchors, mv, 0, bad)
    b0 = s.add_rigid_body(3, 1.0, J1, [1.0, 1.0, 1.2])
    b1 = s.add_rigid_body(7, 2.0, J1, [3.0, 1.0, 1.0])                      # (a turned sphere: R = RYAW)
    for k in (-1, 2):
        _refused(pkg, s, ADMM_ERR_ARG, ["body %d" % k, "not a rigid body"], s.attach_anchors, mv, k, bad)
    for v in (nan, inf, -inf):
        loc = np.zeros((3, 3)); loc[2, 1] = v
        _refused(pkg, s, ADMM_ERR_ARG, ["batch 3", "element 2", "not finite"], s.attach_anchors, mv, b1, loc)
    assert s.attachment(mv)["body"] == -1 and not s.attachment(mv)["local"].any()
    # derived offsets: the restated order from the batch's targets and the body's pose; explicit offsets come back as given
    s.attach_anchors(mv, b1)
    r = s.rigid_state()[b1]
    a = s.attachment(mv)
    assert a["body"] == b1 and a["targets"].tobytes() == (x[free] + 0.01).tobytes()
    assert a["local"].tobytes() == np.array([_local_offset(r.c, r.R, t) for t in x[free] + 0.01]).tobytes()
    back = pkg.attachment_query(c=r.c, R=r.R, local=a["local"])["targets"]
    # ... and return their targets up to the last bits: four rounded operations each way on magnitudes of at most |c| + 2 |t - c|
    assert np.abs(back - a["targets"]).max() <= gamma(8) * 3 * (np.abs(r.c).max() + 2 * np.abs(a["targets"] - r.c).max())
    _refused(pkg, s, ADMM_ERR_ARG, ["batch 3", "attached already", "body 1"], s.attach_anchors, mv, b0, bad)
    # a static batch before finalize: its targets are its nodes' positions
    s.attach_anchors(1, b0)
    idx = np.asarray(pkg.meshgen.bar_anchor_nodes(3, 3))
    r0 = s.rigid_state()[b0]
    assert s.attachment(1)["local"].tobytes() == np.array([_local_offset(r0.c, r0.R, t) for t in x[idx]]).tobytes()
    # update_anchors: the targets of an attached batch are the device's, the flags stay the caller's
    _refused(pkg, s, ADMM_ERR_STATE, ["batch 3", "attached", "body 1"], s.update_anchors, mv, x[free], None)
    _refused(pkg, s, ADMM_ERR_STATE, ["batch 3", "attached"], s.update_anchors, mv, x[free], [1, 0, 1])
    s.update_anchors(mv, active=[1, 0, 1])
    s.detach_anchors(mv)
    s.update_anchors(mv, targets=x[free])
    assert s.attachment(mv)["targets"].tobytes() == x[free].tobytes() and s.attachment(mv)["body"] == -1
    _refused(pkg, s, ADMM_ERR_ARG, ["batch 3", "not attached"], s.detach_anchors, mv)
    _refused(pkg, s, ADMM_ERR_ARG, ["batch 0", "not an anchor batch"], s.detach_anchors, 0)
    _refused(pkg, s, ADMM_ERR_ARG, ["batch 2", "not an anchor batch"], s.attachment, 2)
    loc = np.arange(9.0).reshape(3, 3)
    s.attach_anchors(mv, b0, loc)                                          # attached again, with offsets of the caller's
    assert s.attachment(mv)["local"].tobytes() == loc.tobytes() and s.attachment(mv)["body"] == b0
    Fa, Ta, na = s.attachment_load()
    assert Fa.shape == (2, 3) and not Fa.any() and not Ta.any() and not na.any()           # no frame has run
    s.n_rigid = 1
    _refused(pkg, s, ADMM_ERR_ARG, ["1 rows", "2 rigid bodies"], s.attachment_load)
    s.n_rigid = 2
    s.initialize()                                                         # a host-only context finalizes with attachments
    assert s.attachment(mv)["body"] == b0 and s.attachment(1)["body"] == b0
    _refused(pkg, s, ADMM_ERR_STATE, ["attached"], s.update_anchors, 1, x[idx], None)
    s.detach_anchors(1)
    s.update_anchors(1, targets=x[idx])

    # a sharded context has no body to attach to (add_rigid_body: ADMM_ERR_UNSUPPORTED), so the call ends at the body's check: ARG
    # before UNSUPPORTED, as in add_rigid_body
    t = _host_scene(pkg, world=2)
    t.enable_contact_attribution(True)
    _refused(pkg, t, ADMM_ERR_UNSUPPORTED, ["sharded"], t.add_rigid_body, 3, 1.0, J1, [1.0, 1.0, 1.0])
    _refused(pkg, t, ADMM_ERR_ARG, ["not an anchor batch"], t.attach_anchors, 0, 0, None)
    _refused(pkg, t, ADMM_ERR_ARG, ["not a rigid body"], t.attach_anchors, 1, 0, None)


def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    compile_cpp("attachments", pkg)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _patch(pkg, body, groups, box_c=(0.03, 0.5, 0.02), ball=None):
    """the 9 x 9 patch of test_rigid_bodies (cloth nodes 5 cm apart in the plane y = 0, a collision element on every node) with moving
    anchor batches over the node ranges `groups`; a box of half extents (0.25, 0.05, 0.25), 20 kg, turned by 0.3 rad about y, half a
    metre above the patch: it touches nothing.  `ball`: a second entry, a sphere of 1 kg pressed 4 mm into the patch's last corner.
    `body`: the entries are rigid bodies, the box kicked and spinning, and the batches are attached to the box."""
    n = 9
    g = np.linspace(-0.2, 0.2, n)
    xs = np.array([[g[i], 0.0, g[j]] for j in range(n) for i in range(n)])
    tris = []
    for j in range(n - 1):
        for i in range(n - 1):
            p = i + n * j
            tris += [(p, p + n, p + 1), (p + 1, p + n, p + n + 1)]
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(xs.ravel(), np.full(3 * len(xs), 0.025))
    s.add_forces(KIND["TRI_STRAIN"], np.array(tris, np.int32), [100.0, 0.95, 1.05, 1.0])
    s.att, s.att_nodes = [], {}
    for first, count in groups:
        ids = np.arange(first, first + count, dtype=np.int32)
        k = s.add_forces(KIND["ANCHOR"], ids, [1000.0, 1.0], targets=xs[ids])
        s.att.append(k); s.att_nodes[k] = ids
    s.add_forces(KIND["COLLISION"], np.arange(len(xs), dtype=np.int32), [32.0])
    s.types, s.params = [BOX], [[0.25, 0.05, 0.25, 0.0]]
    s.frames0 = [RYAW + list(box_c)]
    if ball:
        s.types, s.params = s.types + [SPHERE], s.params + [[0.2, 0.046, 0.2, 0.05]]
        s.frames0 = s.frames0 + [EYE + [0.0, 0.0, 0.0]]
    s.set_collision_shapes(s.types, s.params)
    s.set_collision_frames(s.frames0)
    s.enable_contact_attribution(True)
    if body:
        m, h = 20.0, (0.25, 0.05, 0.25)
        J = [m / 3.0 * (h[1] ** 2 + h[2] ** 2), 0.0, 0.0, m / 3.0 * (h[0] ** 2 + h[2] ** 2), 0.0, m / 3.0 * (h[0] ** 2 + h[1] ** 2)]
        b = s.add_rigid_body(0, m, J, list(box_c), [0.0, -1.0, 0.0])
        r = s.rigid_state()[b]
        s.set_rigid_state(b, r.c, r.q, [0.15, -0.1, 0.05], [0.3, 0.4, -0.2])
        if ball:
            s.add_rigid_body(1, 1.0, J1, [0.2, 0.046, 0.2], [0.0, -1.0, 0.0])
        for k in s.att:
            s.attach_anchors(k, b)
    return s


BALL_R, BALL_M = 0.06, 5.0
BALL_C = [0.075, 0.25, 0.556]
BALL_J = [0.4 * BALL_M * BALL_R ** 2 * d for d in (1, 0, 0, 1, 0, 1)]


def _end_nodes(x, na):
    return np.flatnonzero(np.abs(x[:na, 2] - 0.6) < 1e-12).astype(np.int32)


def _bars(pkg, body=True, attach=True, setup=None):
    """the two-bar drop of test_body_collision (bar A a cantilever, bar B dropped across its free half, both surfaces and a floor in the
    list) and a sphere of 5 kg as the list's last entry, beside bar B's long face and 4 mm into it; the 16 nodes of bar A's free end
    are a moving anchor batch (batch 2).  `body`: the sphere is a rigid body under gravity; `attach`: the batch is attached to it -- so
    the body's contact row (bar B) and its attachment row (bar A) are both non-empty."""
    scene = _two_bars(pkg)
    x, tets, anch, m, na, (sa, sb) = scene
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_NH"], tets, [1e5, 1e5, 5])
    s.add_forces(KIND["ANCHOR"], anch, [1000.0, 1.0])
    end = _end_nodes(x, na)
    assert 0 < len(end) < 64
    k = s.add_forces(KIND["ANCHOR"], end, [1000.0, 1.0], targets=x[end])
    s.att, s.att_nodes = [k], {k: end}
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity([0.0, -9.8, 0.0])
    ia = s.add_body_surface(0, na, sa)
    ib = s.add_body_surface(na, len(x) - na, sb)
    s.bodies = [ia, ib]
    s.types = [FLOOR, MESH, MESH, SPHERE]
    s.params = [[0, -0.3, 0, 0], [0, 0, 0, ia], [0, 0, 0, ib], BALL_C + [BALL_R]]
    s.set_collision_shapes(s.types, s.params)
    if setup:
        setup(s)
    s.enable_contact_attribution(True)
    if body:
        s.add_rigid_body(3, BALL_M, BALL_J, BALL_C, G)
        if attach:
            s.attach_anchors(k, 0)
    return s


def _device_against_outside(pkg, make, frames, iters=10, release=None):
    """context A with bodies and attachments on the device; per frame its attached targets must be attachment_query of the old record,
    its attachment rows the sum half of attachment_query fed with batch_reaction and read_local, and its new records rigid_query of the
    old ones and (the contacts' row + the attachment row), in every field.  Context B (make(False)) has neither body nor attachment and
    is moved by the setters and update_anchors(targets = those targets) before every step: x and v of the two must be the same bits.
    release: {frame: {batch: flags}}, handed to both before that frame.  -> per frame (x, v, states, (Fa, Ta, n_active), contact counts)"""
    a, b = make(True), make(False)
    a.initialize(); b.initialize()
    a.set_rigid_depth(DEPTH)
    ne = len(a.types)
    b.frames0 = getattr(b, "frames0", None) or [EYE + [0.0, 0.0, 0.0]] * ne
    att = {k: a.attachment(k) for k in a.att}
    active = {k: np.ones(len(a.att_nodes[k]), np.int32) for k in a.att}
    out = []
    for f in range(frames):
        for k, fl in (release or {}).get(f, {}).items():
            active[k] = np.asarray(fl, np.int32)
            a.update_anchors(k, active=active[k])
        S = a.rigid_state()
        _move_from_outside(b, S, ne)
        tg = {}
        for k in a.att:
            r = S[att[k]["body"]]
            tg[k] = pkg.attachment_query(c=r.c, R=r.R, local=att[k]["local"])["targets"]
            b.update_anchors(k, targets=tg[k], active=active[k])
        a.step(iters); b.step(iters)
        new = a.rigid_state()
        Fa, Ta, na = a.attachment_load()
        for k in a.att:
            on = active[k] != 0
            got = a.attachment(k)["targets"]
            assert got[on].tobytes() == tg[k][on].tobytes(), (f, k)         # (a released element's target is its node's position)
        cnts = None
        for kb, r in enumerate(S):
            Fc, Tc, cnt = a.entry_resultants(pivot=r.c, depth_min=DEPTH)
            row = np.concatenate([Fc[r.entry], Tc[r.entry]])
            mine = [k for k in a.att if att[k]["body"] == kb]
            if mine:
                fe = np.concatenate([a.batch_reaction(k)[0] for k in mine])
                z = np.concatenate([a.read_local(k)["z"] for k in mine])
                q = pkg.attachment_query(f=fe, point=z, active=np.concatenate([active[k] for k in mine]), pivot=r.c)
                assert q["row"].tobytes() == np.concatenate([Fa[kb], Ta[kb]]).tobytes(), (f, kb, q["row"], Fa[kb], Ta[kb])
                assert q["n_active"] == na[kb]
                row = row + q["row"]                                        # one rounded add per component
            else:
                assert np.concatenate([Fa[kb], Ta[kb]]).tobytes() == np.zeros(6).tobytes() and na[kb] == 0
            want = pkg.rigid_query(r, row, DT, count=int(cnt[r.entry]))
            for n in pkg.RIGID_FIELDS:
                assert getattr(want, n).tobytes() == getattr(new[kb], n).tobytes(), (f, kb, n, getattr(want, n), getattr(new[kb], n))
            assert want.count == new[kb].count and new[kb].entry == r.entry, (f, kb)
            assert new[kb].F.tobytes() == (-row[:3]).tobytes() and new[kb].tau.tobytes() == (-row[3:]).tobytes()
            cnts = cnt
        xa, va = a.m_x.copy(), a.m_v.copy()
        assert xa.tobytes() == b.m_x.tobytes(), (f, "x", np.abs(xa - b.m_x).max())
        assert va.tobytes() == b.m_v.tobytes(), (f, "v")
        assert np.isfinite(xa).all()
        out.append((xa, va, new, (Fa, Ta, na), cnts))
    return out, a


@pytest.mark.gpu
def test_patch_on_a_turned_box_device_against_the_rule_from_outside(pkg):
    """scene (a): all 81 nodes of the patch in one batch (a 64-block and a padded one), attached to a turned, spinning box that touches
    nothing: its row is the attachments' alone"""
    res, a = _device_against_outside(pkg, lambda body: _patch(pkg, body, [(0, 81)]), 6)
    print("patch on box: |Fa| %s, |Ta| %s, contacts %s" % (["%.3g" % np.abs(r[3][0][0]).max() for r in res], ["%.3g" % np.abs(r[3][1][0]).max() for r in res], [r[2][0].count for r in res]))
    assert all(r[2][0].count == 0 for r in res) and all(r[3][2][0] == 81 for r in res)
    assert any(np.abs(r[3][0][0]).max() > 0.0 for r in res) and any(np.abs(r[3][1][0]).max() > 0.0 for r in res)
    assert not np.array_equal(res[-1][2][0].R, np.array(RYAW).reshape(3, 3))     # it turned, and the targets with it


@pytest.mark.gpu
def test_bar_end_on_a_sphere_device_against_the_rule_from_outside(pkg):
    """scene (b): bar A's 16 end nodes attached to the sphere, which is in contact with bar B: both rows are non-empty and are added"""
    res, a = _device_against_outside(pkg, lambda body: _bars(pkg, body), 8)
    counts = [r[2][0].count for r in res]
    print("bar end on sphere: contacts %s, Fa_y %s, F_y %s" % (counts, ["%.3g" % r[3][0][0][1] for r in res], ["%.3g" % r[2][0].F[1] for r in res]))
    both = [r for r in res if r[2][0].count > 0 and np.abs(r[3][0][0]).max() > 0.0]
    assert both, counts
    assert all(r[3][2][0] == 16 for r in res)


@pytest.mark.gpu
def test_two_bodies_two_batches_and_releases_device_against_the_rule_from_outside(pkg):
    """scene (c): the box carries a batch of 65 and one of 3 elements -- its sum runs over 68 elements in (batch, element) order, the
    second block holding the last element of the first batch and the whole second one -- and some are released before frame 3; the
    sphere on the patch's corner carries nothing: its attachment row stays +0.0 and its F is minus its contact row, bit for bit"""
    f1 = np.ones(65, np.int32); f1[::7] = 0
    f2 = np.array([1, 0, 1], np.int32)
    make = lambda body: _patch(pkg, body, [(0, 65), (65, 3)], ball=True)
    probe = make(False)
    k1, k2 = probe.att
    del probe
    res, a = _device_against_outside(pkg, make, 7, release={3: {k1: f1, k2: f2}})
    na = [int(r[3][2][0]) for r in res]
    print("two bodies: active attached elements %s, contacts of the sphere %s" % (na, [r[2][1].count for r in res]))
    assert na[:3] == [68] * 3 and na[3:] == [int(f1.sum() + f2.sum())] * 4
    assert max(r[2][1].count for r in res) > 0


@pytest.mark.gpu
def test_a_context_without_a_collision_batch_steps(pkg):
    """a bar whose base nodes are attached to a kicked sphere, no collision batch at all: it steps, the body is loaded by its attachments
    alone and the row is not zero; the record is rigid_query of the attachment row, the contact count stays 0"""
    mg = pkg.meshgen
    x, tets = mg.bar(2, 2, 4)
    m = mg.lumped_tet_mass(x, tets, 200.0)
    base = np.flatnonzero(x[:, 2] == 0.0).astype(np.int32)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets.astype(np.int32), [2e4])
    k = s.add_forces(KIND["ANCHOR"], base, [1000.0, 1.0], targets=x[base])
    c = [0.05, 0.05, -0.2]
    s.set_collision_shapes([SPHERE], [c + [0.05]])
    s.enable_contact_attribution(True)
    M = 10.0
    b = s.add_rigid_body(0, M, [0.4 * M * 0.05 ** 2 * d for d in (1, 0, 0, 1, 0, 1)], c)
    s.attach_anchors(k, b)
    s.initialize()
    r = s.rigid_state()[b]
    s.set_rigid_state(b, r.c, r.q, [0.2, 0.1, -0.3], [0.0, 0.01, 0.0])
    seen = 0.0
    for f in range(4):
        old = s.rigid_state()[b]
        s.step(10)
        Fa, Ta, na = s.attachment_load()
        new = s.rigid_state()[b]
        want = pkg.rigid_query(old, np.concatenate([np.zeros(3) + Fa[b], np.zeros(3) + Ta[b]]), DT, count=0)
        assert want.same_bits(new), f
        assert na[b] == len(base) and np.isfinite(s.m_x).all()
        seen = max(seen, float(np.abs(Fa[b]).max()))
    print("no collision batch: largest |Fa| component %.4g N" % seen)
    assert seen > 0.0


@pytest.mark.gpu
def test_launch_modes_give_the_same_frames(pkg, monkeypatch):
    """scene (b) with ADMM_HIP_GRAPH = 0 (the eager loop), = 1, ADMM_HIP_FRAME_GRAPH = 0 and the default: the same x, v, records and
    attachment rows"""
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = _bars(pkg)
        s.initialize()
        fr = _frames(s, 6)
        assert bool(s.graph_state()["iter_graph"]) == (env.get("ADMM_HIP_GRAPH") != "0")
        res[tuple(env.items())] = (fr, s.rigid_state()[0], np.concatenate([a.ravel() for a in s.attachment_load()[:2]]))
    keys = list(res)
    assert np.abs(res[keys[0]][2]).max() > 0.0
    for k in keys[1:]:
        assert _same_frames(res[keys[0]][0], res[k][0]) and res[keys[0]][1].same_bits(res[k][1]) and res[keys[0]][2].tobytes() == res[k][2].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["tolerance", "anderson", "surface_reaction"])
def test_options_device_against_the_rule_from_outside(pkg, option):
    """an exit by tolerance, Anderson acceleration with window 2, and a surface-reaction share on bar A's surface in scene (b): these
    change the frames themselves, so each is held to the rule applied from outside and to its twin under the same option"""
    setup = dict(tolerance=lambda s: s.set_tolerance(2e-3, 2e-3, 2), anderson=lambda s: s.set_acceleration(2)).get(option)

    def make(body):
        s = _bars(pkg, body, setup=setup)
        if option == "surface_reaction":
            s.set_surface_reaction(s.bodies[1], 0.5)
        return s
    res, a = _device_against_outside(pkg, make, 6, iters=20 if option == "tolerance" else 10)
    assert any(np.abs(r[3][0][0]).max() > 0.0 for r in res)


@pytest.mark.gpu
def test_off_is_off(pkg):
    """a body and an unattached moving-anchor batch: the frames of the same scene built without touching the feature's calls, bit for
    bit -- with the feature's reads made between the frames, and with the batch attached and detached again before the first step"""
    never = _bars(pkg, attach=False); never.initialize()
    read = _bars(pkg, attach=False); read.initialize()
    undone = _bars(pkg, attach=True); undone.detach_anchors(undone.att[0]); undone.initialize()
    k = read.att[0]
    fn, fr, fu = [], [], []
    for f in range(6):
        fn += _frames(never, 1); fu += _frames(undone, 1)
        assert read.attachment(k)["body"] == -1
        fr += _frames(read, 1)
        Fa, Ta, na = read.attachment_load()
        assert not Fa.any() and not Ta.any() and not na.any()
    assert _same_frames(fn, fr) and _same_frames(fn, fu)
    assert never.rigid_state()[0].same_bits(read.rigid_state()[0]) and never.rigid_state()[0].same_bits(undone.rigid_state()[0])
    assert never.rigid_state()[0].count > 0


@pytest.mark.gpu
def test_checkpoint(pkg):
    """4 frames; x, v, every batch's u and warm start, the body's c, q, v, L and the batch's offsets go into a fresh context, which
    attaches after finalize with those offsets; its next 4 frames are those of 8 frames straight"""
    a = _bars(pkg); a.initialize()
    _frames(a, 4)
    X, V = a.m_x.copy(), a.m_v.copy()
    loc = [a.read_local(b) for b in range(4)]
    r = a.rigid_state()[0]
    off = a.attachment(a.att[0])["local"]
    rest = _frames(a, 4)
    b = _bars(pkg, attach=False); b.initialize()
    b.m_x = X; b.m_v = V
    for k, l in enumerate(loc):
        b.write_local(k, u=l["u"], state=l["state"] if l["state"].shape[1] == 4 else None)
    b.set_rigid_state(0, r.c, r.q, r.v, r.L)
    b.attach_anchors(b.att[0], 0, off)
    got = _frames(b, 4)
    assert _same_frames(rest, got)
    assert a.rigid_state()[0].same_bits(b.rigid_state()[0])
    assert np.concatenate(a.attachment_load()[:2]).tobytes() == np.concatenate(b.attachment_load()[:2]).tobytes()


@pytest.mark.gpu
def test_attach_after_finalize_and_detach_mid_run(pkg):
    """two frames unattached, then attach_anchors on the running context with derived offsets (context p) and with the same offsets
    restated on the host from rigid_state and the batch's targets (context q): the same frames; after detach_anchors the targets stay
    where the last frame put them, the attachment row reads zero, the body's F is minus its contact row again and update_anchors takes
    targets again"""
    p, q = _bars(pkg, attach=False), _bars(pkg, attach=False)
    p.initialize(); q.initialize()
    k = p.att[0]
    fp, fq = _frames(p, 2), _frames(q, 2)
    r = q.rigid_state()[0]
    tg = q.attachment(k)["targets"]
    p.attach_anchors(k, 0)
    q.attach_anchors(k, 0, np.array([_local_offset(r.c, r.R, t) for t in tg]))
    assert p.attachment(k)["local"].tobytes() == q.attachment(k)["local"].tobytes()
    fp += _frames(p, 3); fq += _frames(q, 3)
    assert _same_frames(fp, fq) and p.rigid_state()[0].same_bits(q.rigid_state()[0])
    assert np.abs(p.attachment_load()[0]).max() > 0.0
    assert not np.array_equal(p.attachment(k)["targets"], tg)              # the targets rode with the body
    last = p.attachment(k)["targets"]
    p.detach_anchors(k)
    assert p.attachment(k)["body"] == -1 and p.attachment(k)["targets"].tobytes() == last.tobytes()
    old = p.rigid_state()[0]
    p.step(10)
    assert p.attachment(k)["targets"].tobytes() == last.tobytes()
    Fa, Ta, na = p.attachment_load()
    assert not Fa.any() and not Ta.any() and not na.any()
    Fc, Tc, cnt = p.entry_resultants(pivot=old.c, depth_min=0.0)
    assert p.rigid_state()[0].F.tobytes() == (-Fc[3]).tobytes()
    p.update_anchors(k, targets=last + 0.001)
    p.step(10)
    assert p.attachment(k)["targets"].tobytes() == (last + 0.001).tobytes() and np.isfinite(p.m_x).all()


def _hanging(pkg, gravity, kick=None, ball_m=2.0, top_anchored=True, collision=True):
    """a short elastic bar of 2 x 2 x 3 cells of 5 cm hanging along -y from y = 0 (density 1000: 1.5 kg; its bottom layer of 9 nodes
    weighs under 0.3 kg), its top nodes statically anchored when `top_anchored`, its bottom nodes attached to a sphere of `ball_m` kg
    2 cm below them; with `collision` a collision element on every node, nothing in contact"""
    mg = pkg.meshgen
    x0, tets = mg.bar(2, 2, 3)
    x = np.stack([x0[:, 0], -x0[:, 2], x0[:, 1]], 1)                       # a quarter turn about x (orientation kept): z -> -y
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    top = np.flatnonzero(x0[:, 2] == 0.0).astype(np.int32)
    bottom = np.flatnonzero(np.abs(x0[:, 2] - 0.15) < 1e-12).astype(np.int32)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets.astype(np.int32), [2e4])
    if top_anchored:
        s.add_forces(KIND["ANCHOR"], top, [1000.0, 1.0])
    k = s.add_forces(KIND["ANCHOR"], bottom, [1000.0, 1.0], targets=x[bottom])
    if collision:
        s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    if gravity:
        s.add_gravity([0.0, -9.8, 0.0])
    rad = 0.06
    c = [0.05, -0.15 - 0.02 - rad, 0.05]
    s.set_collision_shapes([SPHERE], [c + [rad]])
    s.enable_contact_attribution(True)
    b = s.add_rigid_body(0, ball_m, [0.4 * ball_m * rad ** 2 * d for d in (1, 0, 0, 1, 0, 1)], c, G if gravity else [0.0, 0.0, 0.0])
    s.attach_anchors(k, b)
    s.initialize()
    if kick is not None:
        r = s.rigid_state()[b]
        s.set_rigid_state(b, r.c, r.q, kick, [0.0, 0.0, 0.0])
    return s, x, m, bottom, k, c


@pytest.mark.gpu
def test_linear_momentum_balances_up_to_the_nodes_residual(pkg):
    """No gravity, a free bar carried by a kicked sphere of 2 kg, no collision batch.  Per frame and axis, with P = sum m v + M v_body:
    the body receives dt F = -dt (Fc + Fa) exactly as its record states, so
        P' - P = [sum m dv - dt sum_nodes (f_anchor + f_contact)] + dt [sum_nodes (f_anchor + f_contact) - (Fc + Fa)] + rounding of v'
    The first bracket is the nodes' own residual (the linear solve's and the unconverged iteration's; node_reactions() is the parent's
    report), the only inexact part; the second is one set of numbers summed in two orders.  So |P' - P| <= |first bracket| + rounding:
      the row's two-stage sum is D = 6 + 1 + 7 additions deep (one block, test_query_against_long_double), node_reactions adds one
      element per node (exact) and this test sums in long double: dt gamma(D) sum_i |f_i|
      v' = v + dt (F / M + 0): a division, a product, two additions on the body's side, times M: M gamma(4) (|v| + dt |F| / M)
      one more u each for the conversions and the long double arithmetic.
    The scene has no collision batch on purpose: a collision element that is in no contact still reports f_contact = w^2 (z - x), the
    residue of the unconverged iteration (1e-13 N per node here), which reaches no body; with such elements the drift exceeds the bound
    by dt times their sum (measured: 3e-15 kg m/s in the first frame), a momentum leak of the parent's contact model, not of the
    attachments.
    Printed with -rP: the drift and the residual per frame.  Measured on the MI355X: see DESIGN.md section 3."""
    M = 2.0
    s, x, m, bottom, k, c = _hanging(pkg, gravity=False, kick=[0.3, -0.2, 0.1], ball_m=M, top_anchored=False, collision=False)
    ml = np.asarray(m, LD)[:, None]
    D = 6 + 1 + 7
    v0 = np.asarray(s.m_v, LD).reshape(-1, 3); r0 = s.rigid_state()[0]
    worst = []
    for f in range(8):
        s.step(10)
        v1 = np.asarray(s.m_v, LD).reshape(-1, 3); r1 = s.rigid_state()[0]
        fc, fa, info = s.node_reactions()
        assert info["n_contacts"] == 0 and r1.count == 0 and not np.asarray(fc).any()
        fsum = (np.asarray(fc, LD).reshape(-1, 3) + np.asarray(fa, LD).reshape(-1, 3)).sum(0)
        resid = np.abs((ml * (v1 - v0)).sum(0) - LD(DT) * fsum)
        drift = np.abs((ml * v1).sum(0) + LD(M) * np.asarray(r1.v, LD) - (ml * v0).sum(0) - LD(M) * np.asarray(r0.v, LD))
        fabs = np.abs(np.asarray(fa, LD).reshape(-1, 3)).sum(0)
        rounding = LD(DT) * gamma(D + 1) * fabs + LD(M) * gamma(5) * (np.abs(np.asarray(r0.v, LD)) + LD(DT) * np.abs(np.asarray(r1.F, LD)) / LD(M))
        print("frame %d: momentum drift %s, nodes' residual %s, rounding %s" % (f, drift.astype(float), resid.astype(float), rounding.astype(float)))
        assert np.all(drift <= resid + rounding), (f, drift, resid, rounding)
        assert np.abs(r1.F).max() > 0.0
        worst.append((float(drift.max()), float(resid.max())))
        v0, r0 = v1, r1
    print("linear momentum: largest drift %.3g kg m/s, largest nodes' residual %.3g kg m/s" % (max(w[0] for w in worst), max(w[1] for w in worst)))


@pytest.mark.gpu
def test_a_hanging_sphere_is_arrested_by_the_bar(pkg):
    """Signs and orderings only.  A 2 kg sphere hangs under gravity from the bar, whose top is anchored: over 40 frames its v_y turns
    from negative to positive; at the end its centre is above the bitwise free-fall value of the same frame by more than the bar ever
    stretched; the attachment row pulls the nodes down (Fa_y < 0) while the body's applied F_y is upward; and every attached node stays
    closer to its target than the bar's largest stretch -- the anchors are the stiff part of the chain."""
    frames, M = 40, 2.0
    s, x, m, bottom, k, c0 = _hanging(pkg, gravity=True, ball_m=M)
    v = [0.0, 0.0, 0.0]; c = list(c0)
    vy, stretch, up, down, gap = [], 0.0, False, False, 0.0
    for f in range(frames):
        s.step(10)
        r = s.rigid_state()[0]
        v = [v[j] + DT * ((-0.0) / M + G[j]) for j in range(3)]
        c = [c[j] + DT * v[j] for j in range(3)]
        X = s.m_x.reshape(-1, 3)
        assert np.isfinite(X).all()
        Fa, Ta, na = s.attachment_load()
        vy.append(r.v[1])
        stretch = max(stretch, float((x[bottom, 1] - X[bottom, 1]).mean()))
        down = down or Fa[0][1] < 0.0
        up = up or r.F[1] > 0.0
        gap = max(gap, float(np.linalg.norm(X[bottom] - s.attachment(k)["targets"], axis=1).max()))
        assert r.count == 0 and na[0] == len(bottom)
    first_up = next((i for i, w in enumerate(vy) if w > 0.0), None)
    print("hanging sphere: centre y %.4f against %.4f in free fall, the bar's largest stretch %.4g m, v_y first positive in frame %s, largest node-target distance %.3g m"
          % (r.c[1], c[1], stretch, first_up, gap))
    assert vy[0] < 0.0 and first_up is not None
    assert stretch > 0.0 and r.c[1] - c[1] > stretch
    assert down and up
    assert gap < stretch


@pytest.mark.gpu
def test_class_api_reproduces_the_python_records(pkg, tmp_path):
    """tests/cpp/attachments.cpp: scene (b) through the class mirror (MovingAnchor::body, System::attachment_load) gives the record
    and the attachment row of the Python run after 4 frames, bit for bit"""
    import subprocess
    from test_cpp_host import compile_cpp
    exe = compile_cpp("attachments", pkg)
    x, tets, anch, m, na, (sa, sb) = _two_bars(pkg)
    end = _end_nodes(x, na)
    frames, iters = 4, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(tets), len(anch), na, len(sa), len(sb), len(end)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (tets, anch, sa, sb, end):
            a.astype(np.int32).tofile(f)
        np.array([-0.3, DT] + BALL_C + [BALL_R, BALL_M] + BALL_J + G).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s = _bars(pkg); s.initialize()
    _frames(s, frames, iters)
    want = s.rigid_state()[0].record()
    Fa, Ta, _ = s.attachment_load()
    assert np.abs(Fa[0]).max() > 0.0
    assert open(outp, "rb").read() == bytes(want) + Fa[0].tobytes() + Ta[0].tobytes()
