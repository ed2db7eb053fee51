"""Contact attribution (include/admm_hip.h "contact attribution"; csrc/attribution.hpp, kernels_collision.hpp form 8, kernels_reaction.hpp,
abi_reaction.inc): which entry of the collision list a contact belongs to, the direction of its push, the normal / tangential split of a
reaction and the per-entry resultants.

CPU: attribution_query against a numpy.longdouble restatement; the owners and normals of the ladder scene of
test_collision_form_ladder composed on the host, with the counts that keep the GPU tests from passing vacuously, and a small list where
two entries provably push the same candidates, in both orders; form 8 on all 36 rungs of a host-only context.
GPU: form 8 changes no bit of z and u (every list L0 .. L7, a context without meshes, a context whose only mesh is a plain body surface);
the recorded owners and normals are the host's; frames with the switch on are the frames with it off; the owner records and the per-entry
resultants against the host twins; the compaction's scan boundary; the options; two shards; the C++ class mirror."""
import os
import subprocess
import threading

import numpy as np
import pytest

from checkers import EPS, KIND, gamma
from test_collision_form_ladder import _apply, _compose, _rung, _scene, _system
from test_reactions import _documented_resultant
import test_collision_form_ladder as lad
import test_reactions as trx

L = np.longdouble
ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = 1, 2, 3, 4
FLOOR, SPHERE, MESH, BOX = 0, 1, 3, 4


def _bits_differ(a, b):
    return (np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).any(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 1: the rule against long double
# ---------------------------------------------------------------------------------------------------------------------------------
def _query_inputs():
    rng = np.random.default_rng(23)
    n = 600
    before = rng.normal(size=(n, 3))
    after = before + 0.01 * rng.normal(size=(n, 3))
    f = rng.normal(size=(n, 3)) * rng.uniform(0.1, 100.0, n)[:, None]
    after[:40] = before[:40]                                                # the same bits: not moved
    after[40:80] = before[40:80]
    j = rng.integers(0, 3, 40)
    after[np.arange(40, 80), j] = np.nextafter(before[np.arange(40, 80), j], np.where(rng.uniform(size=40) < 0.5, -np.inf, np.inf))      # one ulp in one coordinate
    before[80:120] = 0.0
    after[80:120] = rng.choice([1e-310, -3e-320, 5e-324, 0.0], (40, 3))
    after[80:120, 0] = 5e-324                                               # (at least one coordinate differs)
    s = np.repeat(rng.choice([1e-150, 1e150], 40), 3).reshape(40, 3)
    before[120:160] *= s; after[120:160] *= s
    nan = np.arange(160, 170)
    after[nan[:5], 1] = np.nan; before[nan[5:], 2] = np.nan
    return before, after, f, nan


def test_attribution_query_against_long_double(pkg):
    """moved: a coordinate's bits differ.  The normal against the long double unit vector of the exact difference: the subtraction rounds
    every component once (the unit vector moves by at most 2 EPS |n_j|), the length takes five operations halved by the root and the
    root's own rounding, the divide one more: |n_j| (gamma(5) / 2 + 4 EPS), no underflow at these scales.  Rows whose squares underflow
    (denormal differences) follow the stated operations exactly as numpy evaluates them in float64 (len = 0: infinite components).
    The split against long double on the returned normal: fn to the dot product's three roundings, gamma(3) sum |f_j n_j|; ft_j to fn's
    error times |n_j| plus the product's and the difference's rounding; fn n + ft gives f back within the same bound.  Rows with the
    same bits: not moved, normal exactly 0, ft = f.  A NaN coordinate: moved, a NaN normal, every other row unaffected."""
    before, after, f, nan = _query_inputs()
    q = pkg.attribution_query(before, after, f)
    n = len(before)
    ok = np.ones(n, bool); ok[nan] = False
    assert np.array_equal(q["moved"][ok], _bits_differ(before, after)[ok])
    assert not q["moved"][:40].any() and q["moved"][40:160].all() and q["moved"][nan].all()
    assert not q["normal"][:40].any() and not np.signbit(q["normal"][:40]).any() and np.array_equal(q["ft"][:40], f[:40]) and not q["fn"][:40].any()
    assert np.isnan(q["normal"][nan]).any(1).all()
    reg = np.concatenate([np.arange(40, 80), np.arange(120, 160), np.arange(170, n)])      # no underflow, no NaN
    d = L(after[reg]) - L(before[reg])
    n_ld = d / np.sqrt((d * d).sum(1))[:, None]
    bound = np.abs(n_ld) * L(0.5 * gamma(5) + 4 * EPS) * (1 + L(gamma(8)))
    err = np.abs(L(q["normal"][reg]) - n_ld)
    print("normal: max error / bound = %.3f" % float((err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all()
    assert (np.abs(np.sqrt((L(q["normal"][reg]) ** 2).sum(1)) - 1) <= 4 * EPS).all()
    with np.errstate(all="ignore"):                                         # the denormal rows: the stated operations in float64
        dd = after[80:120] - before[80:120]
        ln = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        assert np.array_equal(q["normal"][80:120], dd / ln[:, None], equal_nan=True) and (ln == 0).all()
    fin = ok & np.isfinite(q["normal"]).all(1)
    nr, ff = L(q["normal"][fin]), L(f[fin])
    fn_ld = (ff * nr).sum(1)
    b_fn = L(gamma(3)) * (np.abs(ff * nr)).sum(1)
    assert (np.abs(L(q["fn"][fin]) - fn_ld) <= b_fn).all()
    ft_ld = ff - fn_ld[:, None] * nr
    b_ft = ((np.abs(nr) * b_fn[:, None] + L(EPS) * np.abs(fn_ld[:, None] * nr)) * (1 + L(EPS)) + L(EPS) * np.abs(ft_ld)) * (1 + L(gamma(4)))
    assert (np.abs(L(q["ft"][fin]) - ft_ld) <= b_ft).all()
    back = L(q["fn"][fin])[:, None] * nr + L(q["ft"][fin])
    assert (np.abs(back - ff) <= b_ft).all()
    assert fin.sum() > 400
    # the NaN rows do not touch the others; the split about given normals is the same operation
    b2, a2 = before.copy(), after.copy()
    b2[nan] = 0.0; a2[nan] = 1.0
    q2 = pkg.attribution_query(b2, a2, f)
    for key in ("moved", "normal", "fn", "ft"):
        assert np.array_equal(q[key][ok], q2[key][ok], equal_nan=True), key
    q3 = pkg.attribution_query(f=f[fin], normal=q["normal"][fin])
    assert np.array_equal(q3["fn"], q["fn"][fin]) and np.array_equal(q3["ft"], q["ft"][fin]) and not q3["moved"].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 2: owners on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _compose_pre(pkg, C, k, sides=None):
    """_compose restated with, per entry, the point before its rule and the point behind it before friction -> (z, [(before, pre)])"""
    H = lad._host_meshes(pkg, C)
    el = C["elems"]
    x0, v0 = C["x0"][el], C["v0"]
    p = C["dx"] + C["u"]
    is_tet = (el >= C["o_t"]) & (el < C["o_f"])
    is_bar = (el >= C["o_b"]) & (el < C["o_t"])
    vid_s, vid_b = C["vid_sheet"], C["vid_body"]
    steps = []
    for e in C["lists"][k]:
        ty, par, f, mu, mi = e["ty"], e["par"], e["frame"], e["mu"], e["mesh"]
        framed = not np.array_equal(f, lad.IDENT)
        t = par[:3]
        vi = None
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
            moved = moved.astype(bool)
        elif mi in (lad.ICO, lad.CUBE):
            proj, sd = H[mi].query(p, t, frame=f if framed else None)
            moved = sd > 0
            q = np.where(moved[:, None], proj, p)
            if mi == lad.ICO and k >= 2:
                vi = pkg.mesh_velocity_query(H[mi], None, lad._to_local(f, p) if framed else p, C["vel_ico"], t)[0]
                if framed:
                    vi = lad._rotate(f, vi)
        elif mi == lad.TET:
            proj, sd = H[lad.TET].query(p)
            moved = (sd > 0) & ~is_tet
            q = np.where(moved[:, None], proj, p)
            mu = lad.MU_TET if k >= 2 else 0.0
            vi = pkg.mesh_velocity_query(H[lad.TET], None, p, v0[H["tet_nodes"]])[0]
        elif mi == lad.SHELL:
            proj, sd = H[lad.SHELL].query(p, t)
            moved = (proj != p).any(1)
            q = np.where(moved[:, None], proj, p)
            vi = pkg.mesh_velocity_query(H[lad.SHELL], None, p, C["vel_shell"], t)[0]
        elif mi == lad.SHEET:
            q, sd, _ = H[lad.SHEET].query_excluding(p, vid_s, t)
            moved = sd > 0
            mu = lad.MU_SHEET
            vi = H[lad.SHEET].velocity_query_excluding(p, vid_s, v0[:C["ns"]], t)[0]
        elif mi == lad.MEM:
            q = H[lad.MEM].query_sided(p, sides[el], lad.MEM_REACH, t)[0]
            moved = (q != p).any(1)
        else:
            assert mi == lad.BODY
            q = p.copy()
            sf = is_bar & (vid_b >= 0)
            qs, sd, tri, _ = H[lad.BODY].query_self(p[sf], vid_b[sf], H["rest"], *lad.tb.LENGTHS)
            q[sf] = qs
            moved = np.zeros(len(p), bool); moved[sf] = (sd > 0) & (tri >= 0)
            pf, sdf = H[lad.BODY].query(p[~is_bar])
            q[~is_bar] = np.where((sdf > 0)[:, None], pf, p[~is_bar])
            moved[~is_bar] = sdf > 0
            mu = lad.MU_BODY
            vel = v0[H["body_nodes"]]
            vi = np.zeros_like(p)
            vi[sf] = H[lad.BODY].velocity_query_self(p[sf], vid_b[sf], H["rest"], lad.tb.REACH, lad.tb.RHO, vel)[0]
            vi[~is_bar] = pkg.mesh_velocity_query(H[lad.BODY], None, p[~is_bar], vel)[0]
        steps.append((p, q))
        if k >= 1 and mu > 0:
            w = lad._np_rigid(e["motion"], q)
            if vi is not None:
                w = w + lad.DT * vi
            q2, _ = pkg.friction_query_moving(p, q, x0, w, mu)
            q = np.where(moved[:, None], q2, q)
        p = q
    return p, steps


_HOST = {}


def _host_owners(pkg, k, sides=None):
    """-> dict(z, owner [n], normal [n][3], movers [n]: how many entries moved the element) of list Lk, composed on the host"""
    C = _scene(pkg)
    sides = lad._host_sides(pkg, C) if sides is None else sides
    key = (k, sides.tobytes())
    if key not in _HOST:
        z, steps = _compose_pre(pkg, C, k, sides)
        n = len(z)
        owner = np.full(n, -1, np.int32); normal = np.zeros((n, 3)); movers = np.zeros(n, int)
        for e, (before, pre) in enumerate(steps):
            q = pkg.attribution_query(before, pre)
            owner[q["moved"]] = e
            normal[q["moved"]] = q["normal"][q["moved"]]
            movers += q["moved"]
        _HOST[key] = dict(z=z, owner=owner, normal=normal, movers=movers)
    return _HOST[key]


def test_owners_on_the_host(pkg):
    """the restatement gives _compose's z bit for bit on all eight lists, so its pre-friction points are those of the composition; from
    them: every entry of every list owns at least 10 elements and at least 100 elements have no owner; an owner's normal is a unit vector,
    no owner an exact zero.  The elements that two or more entries moved, where the owner is provably the later one, are counted and
    printed per list: the ladder's clusters sit at one obstacle each, so the lower lists have none -- that condition is met by the
    dedicated list of test_owner_is_the_later_of_two_movers, on the host and on the device, and by L6 and L7 (at least 10 each)."""
    C = _scene(pkg)
    sides = lad._host_sides(pkg, C)
    for k in range(8):
        h = _host_owners(pkg, k)
        want, _ = _compose(pkg, C, k, sides)
        assert np.array_equal(h["z"].view(np.uint64), want.view(np.uint64)), k
        ne = len(C["lists"][k])
        owned = np.bincount(h["owner"][h["owner"] >= 0], minlength=ne)
        multi = int((h["movers"] >= 2).sum())
        print("L%d: owned per entry %s, no owner %d, moved by two or more %d" % (k, owned.tolist(), int((h["owner"] < 0).sum()), multi))
        assert (owned >= 10).all(), (k, owned)
        assert (h["owner"] < 0).sum() >= 100
        if k >= 6:                                                                       # (the memory shell and the body lie over other obstacles)
            assert multi >= 10, (k, multi)
        has = h["owner"] >= 0
        assert (np.abs(np.sqrt((L(h["normal"][has]) ** 2).sum(1)) - 1) <= 4 * EPS).all() and not h["normal"][~has].any()
        assert ((h["movers"] > 0) == has).all()


# a floor and a sphere that overlap it, in both orders, plus a box under a frame: candidates inside the sphere AND under the floor are pushed by both
PAIR_FLOOR, PAIR_SPH = [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.5]
PAIR_BOX, PAIR_FRAME = [0.2, 0.1, 0.3, 0.0], lad._frame(lad._rot([0.2, 0.1, 1.0], 0.6), [2.0, 0.0, 0.0])


def _pair_candidates():
    rng = np.random.default_rng(5)
    d = rng.normal(size=(40, 3)); d[:, 1] = -np.abs(d[:, 1]) - 0.3                       # the lower half of the sphere, well under the floor
    both = 0.45 * rng.uniform(0.3, 0.9, 40)[:, None] * d / np.linalg.norm(d, axis=1)[:, None]
    up = both[:20] * [1.0, -1.0, 1.0]                                                   # the upper half: the sphere alone
    under = np.stack([rng.uniform(1.0, 1.5, 20), -rng.uniform(0.01, 0.1, 20), rng.uniform(-1, 1, 20)], 1)      # the floor alone
    inbox = np.array([2.0, 0.0, 0.0]) + np.abs(rng.uniform(0.0, 0.05, (20, 3)))         # at the turned box's centre, on and above the floor
    free = np.stack([rng.uniform(3.0, 4.0, 30), rng.uniform(0.5, 1.0, 30), rng.uniform(-1, 1, 30)], 1)
    return np.concatenate([both, up, under, inbox, free])


def _pair_lists():
    fl, sp, bx = (FLOOR, PAIR_FLOOR, lad.IDENT), (SPHERE, PAIR_SPH, lad.IDENT), (BOX, PAIR_BOX, PAIR_FRAME)
    return {"floor, sphere, box": [fl, sp, bx], "sphere, floor, box": [sp, fl, bx]}


def _pair_host(pkg, entries, p):
    owner = np.full(len(p), -1, np.int32); normal = np.zeros((len(p), 3)); movers = np.zeros(len(p), int)
    for e, (ty, par, fr) in enumerate(entries):
        q, _ = pkg.shape_query(ty, par, p, fr)
        a = pkg.attribution_query(p, q)
        owner[a["moved"]] = e; normal[a["moved"]] = a["normal"][a["moved"]]; movers += a["moved"]
        p = q
    return p, owner, normal, movers


def test_owner_is_the_later_of_two_movers(pkg):
    """the first 40 candidates are inside the sphere's lower half and under the floor: whichever entry comes first pushes them, and the
    other pushes the result again (both provably: the floor lifts a point to y = 0 inside the sphere, the sphere's surface below the
    floor is below y = 0), so the owner is entry 1 in both orders -- the sphere in one, the floor in the other: it flips with the order.
    The box under its frame owns the candidates at its centre in both."""
    p = _pair_candidates()
    res = {name: _pair_host(pkg, E, p) for name, E in _pair_lists().items()}
    (_, o_fs, n_fs, m_fs), (_, o_sf, n_sf, m_sf) = res["floor, sphere, box"], res["sphere, floor, box"]
    assert (m_fs[:40] == 2).all() and (m_sf[:40] == 2).all() and (o_fs[:40] == 1).all() and (o_sf[:40] == 1).all()
    assert np.array_equal(n_sf[:40], np.tile([0.0, 1.0, 0.0], (40, 1))) and (np.abs(n_fs[:40, [0, 2]]).max(1) > 0).all()      # the floor's normal / the sphere's radial
    assert (o_fs[40:60] == 1).all() and (o_sf[40:60] == 0).all() and (o_fs[60:80] == 0).all() and (o_sf[60:80] == 1).all()
    assert (o_fs[80:100] == 2).all() and (o_sf[80:100] == 2).all() and (o_fs[100:] == -1).all() and (o_sf[100:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 3: the form with the switch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_form_8_on_every_rung_of_a_host_only_context(pkg):
    """collision_form_of takes the switch: form 8 for Lk + Tj of all 36 rungs, j again when the switch is off; the reports refuse a
    host-only context like every compute call"""
    C = _scene(pkg)
    s = _system(pkg, C, -1)
    for k in range(8):
        for j in range(k, 8):
            _apply(s, C, k, j)
            s.enable_contact_attribution()
            assert s.collision_form() == 8, (k, j)
            s.enable_contact_attribution(False)
            assert s.collision_form() == j, (k, j)
    s.enable_contact_attribution()
    assert trx._code(pkg, s.batch_contact_owner, s.batch) == ERR_HIP and trx._code(pkg, s.contact_owners) == ERR_HIP
    assert trx._code(pkg, s.batch_contact_owner, 0) == ERR_UNSUPPORTED and trx._code(pkg, s.contact_owners, depth_min=-1.0) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 4, 5: form 8 changes no bit, and records the host's owners
# ---------------------------------------------------------------------------------------------------------------------------------
_ATT = {}


def _att_rung(pkg, k):
    """one local step of the collision batch with attribution on, on list Lk, from the state of _rung, on a context of its own ->
    dict(z, u, owner, normal, filled: the record right after the switch, cleared: after a second local step that touches nothing)"""
    C = _scene(pkg)
    if "s" not in _ATT:
        s = _ATT["s"] = _system(pkg, C, 0)
        _apply(s, C, 0, 0)
        s.step(1)                                                                        # (the reports are those of a context that has stepped)
    s = _ATT["s"]
    if k not in _ATT:
        s.enable_contact_attribution(False)
        _apply(s, C, k, k)
        assert s.collision_form() == k
        s.enable_contact_attribution()
        assert s.collision_form() == 8
        filled = s.batch_contact_owner(s.batch)
        s.m_x = C["x0"].ravel()
        s.m_v = C["v0"].ravel()
        s.write_local(s.batch, u=C["u"])
        s.set_collision_sides(lad.MEM, C["sides0"])
        s.latch_collision_sides()
        s.local_step_dx(s.batch, C["dx"])
        r = s.read_local(s.batch)
        out = dict(z=r["z"].copy(), u=r["u"].copy(), filled=filled, sides=s.collision_sides(lad.MEM))
        out["owner"], out["normal"] = s.batch_contact_owner(s.batch)
        far = np.array([0.0, 30.0, 0.0]) + 0.01 * np.random.default_rng(k).normal(size=C["dx"].shape)
        s.write_local(s.batch, u=np.zeros_like(C["u"]))
        s.local_step_dx(s.batch, far)
        out["cleared"] = s.batch_contact_owner(s.batch)
        assert np.array_equal(s.read_local(s.batch)["z"], far)
        _ATT[k] = out
    return _ATT[k]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(8))
def test_form_8_changes_no_bit(pkg, k):
    """list Lk with attribution on: z and u of the 887 elements bitwise those of form k"""
    zk, uk, _ = _rung(pkg, k, k)
    a = _att_rung(pkg, k)
    assert np.array_equal(a["z"], zk), np.flatnonzero((a["z"] != zk).any(1))
    assert np.array_equal(a["u"], uk)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(8))
def test_recorded_owners_and_normals(pkg, k):
    """batch_contact_owner equals the host's owners exactly and the host's normals bitwise; the switch fills -1 and 0.0; a second local
    step from candidates that touch nothing rewrites every owner to -1 and every normal to 0.0"""
    a = _att_rung(pkg, k)
    h = _host_owners(pkg, k, a["sides"])
    n = len(h["owner"])
    assert np.array_equal(a["filled"][0], np.full(n, -1, np.int32)) and not a["filled"][1].any()
    bad = np.flatnonzero(a["owner"] != h["owner"])
    assert bad.size == 0, (bad, a["owner"][bad], h["owner"][bad])
    assert np.array_equal(a["normal"].view(np.uint64), h["normal"].view(np.uint64)), np.flatnonzero((a["normal"] != h["normal"]).any(1))
    assert (a["owner"] >= 0).sum() >= 100
    assert np.array_equal(a["cleared"][0], np.full(n, -1, np.int32)) and not a["cleared"][1].any()


def _step_pair(s, bt, C, on, surfaces=False):
    """one local step of batch bt from the ladder's state with the switch on or off -> (z, u); surfaces: the context has body surfaces,
    which follow m_x and m_v"""
    s.enable_contact_attribution(on)
    s.m_x = C["x0"].ravel()
    s.write_local(bt, u=C["u"])
    if surfaces:
        s.m_v = C["v0"].ravel()
        s.latch_collision_sides()
    s.local_step_dx(bt, C["dx"])
    r = s.read_local(bt)
    return r["z"].copy(), r["u"].copy()


@pytest.mark.gpu
def test_form_8_without_meshes(pkg):
    """a context without meshes (the <8, false> instantiation) on the analytic entries of L0 .. L3: form 8 gives the bits of form k, and
    with the switch off again the form is k"""
    C = _scene(pkg)
    a = pkg.System(device_id=0)
    a.set_timestep(lad.DT)
    a.add_nodes(C["xr"].ravel(), np.ones(3 * C["n"]))
    b = a.add_forces(KIND["COLLISION"], C["elems"], [lad.W])
    a.initialize()
    for k in range(4):
        E = lad._analytic(C, k)
        a.enable_contact_attribution(False)
        a.set_collision_shapes([], np.zeros((0, 4)))
        a.set_collision_shapes([e["ty"] for e in E], [e["par"] for e in E])
        if k >= 1:
            a.set_collision_friction([e["mu"] for e in E])
            a.set_collision_motion([e["motion"] for e in E])
            a.set_collision_frames([e["frame"] for e in E])
        assert a.collision_form() == k
        z0, u0 = _step_pair(a, b, C, False)
        z8, u8 = _step_pair(a, b, C, True)
        assert a.collision_form() == 8
        assert (z0 != C["dx"] + C["u"]).any(1).sum() >= 100
        assert np.array_equal(z8, z0) and np.array_equal(u8, u0), k


@pytest.mark.gpu
def test_form_8_on_a_plain_body_surface(pkg):
    """a context whose only mesh is a plain body surface -- no shell, no memory, no self-collision, so every device table of forms 4 to 7
    is null --: form 8 gives the bits of the list's own form 0 (project_collision_mesh_kernel), and the tet body's entry moves candidates"""
    C = _scene(pkg)
    s = pkg.System(device_id=0)
    s.set_timestep(lad.DT)
    s.add_nodes(C["xr"].ravel(), np.ones(3 * C["n"]))
    s.add_forces(KIND["TET_LINEAR"], C["tets_t"] + C["o_t"], [2e4])
    b = s.add_forces(KIND["COLLISION"], C["elems"], [lad.W])
    mid = s.add_body_surface(C["o_t"], C["nt"], C["Ft"] + C["o_t"])
    s.set_collision_shapes([FLOOR, MESH], [[0, lad.FLOOR_Y, 0, 0], [0, 0, 0, mid]])
    s.initialize()
    assert s.collision_form() == 0
    z0, u0 = _step_pair(s, b, C, False, surfaces=True)
    z8, u8 = _step_pair(s, b, C, True, surfaces=True)
    assert s.collision_form() == 8 and s.body_surface_status(mid)["refused"] == 0
    p = C["dx"] + C["u"]
    floor = pkg.shape_query(FLOOR, [0, lad.FLOOR_Y, 0, 0], p)[0]
    assert (z0 != floor).any(1).sum() >= 10                                             # moved by the body surface
    assert np.array_equal(z8, z0) and np.array_equal(u8, u0)


@pytest.mark.gpu
def test_owner_flips_with_the_order_on_the_device(pkg):
    """the dedicated lists of test_owner_is_the_later_of_two_movers on the device: z, owners and normals are the host's, bit for bit, in
    both orders -- 40 candidates that both the floor and the sphere push are owned by whichever comes later"""
    p = _pair_candidates()
    n = len(p)
    s = pkg.System(device_id=0)
    s.set_timestep(lad.DT)
    s.add_nodes(p.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [lad.W])
    s.initialize()
    s.step(1)                                                                            # (the reports are those of a context that has stepped)
    s.enable_contact_attribution()
    owners = []
    for name, E in _pair_lists().items():
        s.set_collision_shapes([], np.zeros((0, 4)))
        s.set_collision_shapes([e[0] for e in E], [e[1] for e in E])
        s.set_collision_frames([e[2] for e in E])
        assert s.collision_form() == 8
        s.write_local(b, u=np.zeros((n, 3)))
        s.local_step_dx(b, p)
        z, owner, normal, movers = _pair_host(pkg, E, p)
        ow, nr = s.batch_contact_owner(b)
        assert np.array_equal(s.read_local(b)["z"], z), name
        assert np.array_equal(ow, owner) and np.array_equal(nr.view(np.uint64), normal.view(np.uint64)), name
        assert (movers[:40] == 2).all() and (ow[:40] == 1).all()
        owners.append(ow)
    assert (owners[0][40:80] != owners[1][40:80]).all()                                   # the single movers' owner follows the entry's place


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 6, 7: frames, the owner records and the per-entry resultants
# ---------------------------------------------------------------------------------------------------------------------------------
_FR = {}


def _frames(pkg):
    """two identical contexts on L7 with gravity, three frames of step(10), attribution on in the first"""
    if _FR:
        return _FR
    C = _scene(pkg)
    ss = []
    for on in (True, False):
        s = _system(pkg, C, 0, gravity=True)
        _apply(s, C, 7, 7)
        if on:
            s.enable_contact_attribution()
        assert s.collision_form() == (8 if on else 7)
        s.m_x = C["x0"].ravel()
        s.m_v = C["v0"].ravel()
        ss.append(s)
    fr = [[], []]
    for _ in range(3):
        for s, f in zip(ss, fr):
            s.step(10)
            f.append((s.m_x.copy(), s.m_v.copy()))
    _FR.update(on=ss[0], off=ss[1], frames=fr, graph=[s.graph_state() for s in ss])
    return _FR


@pytest.mark.gpu
def test_frames_with_attribution_are_the_frames_without(pkg):
    """m_x and m_v bitwise equal after every frame, the frame graph replayed form 8; then the switch off (form 7) and on again (form 8)
    between frames: the frames stay equal"""
    F = _frames(pkg)
    C = _scene(pkg)
    assert lad._same_frames(F["frames"][0], F["frames"][1])
    assert F["graph"][0]["frame_graph_iters"] == 10 and F["graph"][0]["graph_launches"] >= 2, F["graph"][0]
    assert np.abs(F["frames"][0][-1][0] - C["x0"].ravel()).max() > 1e-2
    a, b = F["on"], F["off"]
    if "toggled" not in F:
        for on, form in ((False, 7), (True, 8)):
            a.enable_contact_attribution(on)
            assert a.collision_form() == form and a.graph_state()["frame_graph_iters"] == 0      # the captured graphs went with the form
            a.step(10); b.step(10)
            assert np.array_equal(a.m_x, b.m_x) and np.array_equal(a.m_v, b.m_v), on
        F["toggled"] = True
    assert a.graph_state()["frame_graph_iters"] == 10


@pytest.mark.gpu
def test_contact_owner_records_and_entry_resultants(pkg):
    """after the frames: contact_owners lists the nodes of contacts in its order; a record's entry and normal are those of the node's
    collision element (one per node in this scene); the split is attribution_query of the contact's f about that normal, bit for bit;
    row q of entry_resultants is the documented two-stage sum over exactly the contacts with entry q, the last row those with entry -1,
    bit for bit; the counts add up to contact_resultant's.  The rows' sum against contact_resultant: the two are tree sums of the same
    terms in different orders, each off the exact sum by at most (its depth) EPS sum |terms| with a depth of at most 6 + 8 + blocks / 256
    additions, and the rows are added here in long double; (count + n_entries) EPS sum |terms| covers both."""
    F = _frames(pkg)
    test_frames_with_attribution_are_the_frames_without(pkg)
    s, C = F["on"], _scene(pkg)
    ne = len(C["lists"][7])
    owner, normal = s.batch_contact_owner(s.batch)
    pivot = (0.3, -0.1, 0.4)
    for dm in (1e-10, 1e-4):
        c = s.contacts(depth_min=dm)
        o = s.contact_owners(depth_min=dm)
        assert len(c) >= 50 and np.array_equal(o["node"], c["node"]) and s.last_contact_count == len(c)
        assert np.array_equal(o["entry"], owner[c["node"]]) and np.array_equal(o["normal"].view(np.uint64), normal[c["node"]].view(np.uint64))
        q = pkg.attribution_query(f=c["f"], normal=o["normal"])
        assert np.array_equal(o["f_normal"], q["fn"]) and np.array_equal(o["f_tangent"], q["ft"])
        assert np.array_equal(s.contact_owners(depth_min=dm, capacity=7), o[:7])
        force, torque, count = s.entry_resultants(pivot=pivot, depth_min=dm)
        got = np.concatenate([force, torque], 1)
        print("depth_min %g: contacts per entry %s" % (dm, count.tolist()))
        for row in range(ne + 1):
            flag = o["entry"] == (row if row < ne else -1)
            assert count[row] == flag.sum()
            assert np.array_equal(got[row], _documented_resultant(c["f"], c["point"], pivot, flag)), (dm, row)
        tf, tt, tc = s.contact_resultant(pivot=pivot, depth_min=dm)
        assert count.sum() == tc == len(c)
        r = c["point"] - np.asarray(pivot)
        terms = np.concatenate([c["f"], np.stack([r[:, 1] * c["f"][:, 2] - r[:, 2] * c["f"][:, 1], r[:, 2] * c["f"][:, 0] - r[:, 0] * c["f"][:, 2],
                                                  r[:, 0] * c["f"][:, 1] - r[:, 1] * c["f"][:, 0]], 1)], 1)
        bound = (tc + ne) * L(EPS) * np.abs(L(terms)).sum(0)
        diff = np.abs(L(got).sum(0) - L(np.concatenate([tf, tt])))
        print("rows against contact_resultant: max difference / bound = %.3g" % float((diff / bound).max()))
        assert (diff <= bound).all()
    assert (count[:ne] > 0).sum() >= 3 and count[0] > 0                                  # several obstacles carry something, the floor among them
    assert trx._code(pkg, s.entry_resultants, n_entries=ne - 1) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 8: the scan boundary
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scan_boundary_with_two_entries(pkg):
    """128 * 64 + 1 free particles (one count block more than one pass of the scan covers): the first half drops on a floor at y = 2
    (entry 0), the second on a box whose top is at y = 2.5 (entry 1, under a frame that only translates), disjoint footprints.  After two
    frames every contact of the first group has entry 0 and normal (0, 1, 0) exactly, every contact of the second entry 1 with an upward
    normal; the per-entry counts are the groups' sizes in contact; the rows are the host sums bit for bit"""
    N = trx.N_BIG
    h = N // 2
    rng = np.random.default_rng(77)
    x0 = np.stack([rng.uniform(1.0, 2.0, N), trx.FLOOR_Y + rng.uniform(0.02, 0.1, N), rng.uniform(1.0, 2.0, N)], 1)
    x0[h:, 0] += 3.0; x0[h:, 1] += 0.5
    v0 = np.stack([rng.uniform(-0.2, 0.2, N), np.full(N, -5.0), rng.uniform(-0.2, 0.2, N)], 1)
    s = pkg.System(device_id=0)
    s.set_timestep(trx.DT)
    s.add_nodes(x0.ravel(), np.repeat(rng.uniform(0.5, 2.0, N), 3))
    coll = s.add_forces(KIND["COLLISION"], np.arange(N, dtype=np.int32), [trx.W_COLL])
    s.add_gravity(trx.G)
    s.set_collision_shapes([FLOOR, BOX], [[0.0, trx.FLOOR_Y, 0.0, 0.0], [1.5, 0.5, 1.5, 0.0]])
    s.set_collision_frames([lad.IDENT, lad._frame(np.eye(3), [4.5, trx.FLOOR_Y, 1.5])])
    s.enable_contact_attribution()                                                       # before initialize: finalize allocates the record
    s.initialize()
    s.m_v = v0.ravel()
    assert s.collision_form() == 8
    for _ in range(2):
        s.step(10)
    c, o = s.contacts(), s.contact_owners()
    assert np.array_equal(o["node"], c["node"]) and len(c) > 0.9 * N
    first = o["node"] < h
    assert first.sum() > 0.9 * h and (~first).sum() > 0.9 * (N - h)
    assert (o["entry"][first] == 0).all() and np.array_equal(o["normal"][first], np.tile([0.0, 1.0, 0.0], (first.sum(), 1)))
    assert (o["entry"][~first] == 1).all() and (o["normal"][~first, 1] > 0.99).all()
    assert np.array_equal(o["f_normal"][first], c["f"][first, 1]) and (c["point"][~first, 1] >= trx.FLOOR_Y + 0.5 - 1e-12).all()
    pivot = (1.5, 2.0, 1.5)
    force, torque, count = s.entry_resultants(pivot=pivot)
    assert count.tolist() == [first.sum(), (~first).sum(), 0]
    got = np.concatenate([force, torque], 1)
    for row, flag in enumerate((first, ~first, np.zeros(len(c), bool))):
        assert np.array_equal(got[row], _documented_resultant(c["f"], c["point"], pivot, flag)), row
    assert not got[2].any() and got[0, 1] > 0 and got[1, 1] > 0
    ow, nr = s.batch_contact_owner(coll)
    assert np.array_equal(ow[c["node"]], o["entry"]) and np.array_equal(nr[c["node"]], o["normal"])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 9: options
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_state_and_argument_errors(pkg):
    """ADMM_ERR_STATE from every report while the switch is off and before the first step; ADMM_ERR_ARG for a wrong n_entries and a
    negative or NaN depth_min; ADMM_ERR_UNSUPPORTED for batch_contact_owner on the anchor batch"""
    s = trx._particles(pkg, 65)
    reports = ((s.batch_contact_owner, (s.coll,)), (s.contact_owners, ()), (s.entry_resultants, ()))
    for fn, a in reports:
        assert trx._code(pkg, fn, *a) == ERR_STATE                                       # off, no step
    s.enable_contact_attribution()
    for fn, a in reports:
        assert trx._code(pkg, fn, *a) == ERR_STATE                                       # on, no step
    s.enable_contact_attribution(False)
    s.step(10)
    for fn, a in reports:
        assert trx._code(pkg, fn, *a) == ERR_STATE                                       # stepped, off
    assert trx._code(pkg, s.batch_contact_owner, s.anch) == ERR_UNSUPPORTED
    s.enable_contact_attribution()
    ow, nr = s.batch_contact_owner(s.coll)
    assert (ow == -1).all() and not nr.any()                                             # the switch cleared the record
    for dm in (-1.0, -1e-300, float("nan")):
        assert trx._code(pkg, s.contact_owners, depth_min=dm) == ERR_ARG and trx._code(pkg, s.entry_resultants, depth_min=dm) == ERR_ARG
    for ne in (0, 1, 3, 65):
        assert trx._code(pkg, s.entry_resultants, n_entries=ne) == ERR_ARG
    assert trx._code(pkg, s.batch_contact_owner, s.anch) == ERR_UNSUPPORTED
    assert s.L.admm_hip_batch_contact_owner(s.h, 99, None, None) == ERR_ARG and s.L.admm_hip_get_contact_owners(s.h, 0.0, None, 4, None) == ERR_ARG
    s.step(10)
    assert len(s.contact_owners()) == len(s.contacts()) == 32 and s.entry_resultants()[2].sum() == 32


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["tolerance", "acceleration"])
def test_records_under_the_solvers_options(pkg, option):
    """a tolerance exit after three of ten iterations, and Anderson acceleration at window 3: the last local step's input (the iterate
    before the last solve) is not kept, so the record cannot be recomputed on the host; what must hold for the record of any local step:
    an owner names an entry of the list and has a unit normal to 2 ulp, no owner has a zero normal; a floor owner's normal is (0, 1, 0)
    exactly; both entries own contacts, and the owner records still split f_contact by attribution_query's bits"""
    s = trx._particles(pkg, 65)
    s.enable_contact_attribution()
    if option == "tolerance":
        s.set_tolerance(1e300, 1e300, 3)
    else:
        s.set_acceleration(3)
    s.step(10)
    if option == "tolerance":
        assert s.residuals()[2] == 3
    else:
        log = s.acceleration_log()
        assert len(log) == 10 and any(r["extrapolated"] for r in log)
    ow, nr = s.batch_contact_owner(s.coll)
    has = ow >= 0
    assert set(np.unique(ow)) <= {-1, 0, 1} and (ow == 0).sum() >= 10 and (ow == 1).sum() >= 1, np.bincount(ow + 1)
    assert (np.abs(np.sqrt((L(nr[has]) ** 2).sum(1)) - 1) <= 2 * 2 * EPS).all() and not nr[~has].any()
    assert np.array_equal(nr[ow == 0], np.tile([0.0, 1.0, 0.0], ((ow == 0).sum(), 1)))
    c, o = s.contacts(), s.contact_owners()
    assert len(c) == 32 and np.array_equal(o["node"], c["node"]) and np.array_equal(o["entry"], ow[c["node"]])
    q = pkg.attribution_query(f=c["f"], normal=o["normal"])
    assert np.array_equal(o["f_normal"], q["fn"]) and np.array_equal(o["f_tangent"], q["ft"])


@pytest.mark.gpu
def test_two_shards_record_their_local_elements(pkg, monkeypatch):
    """two contexts on one GPU with threads, as test_reactions starts them, the switch set before they are initialized together: each
    rank's batch_contact_owner covers its local elements; put together by local_elements they are the one-rank record (the floor's
    normal is exact, and no node of this bar is within the shards' 1e-9 of the floor's decision)"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "8")
    tet = ("TET_LINEAR", [1e5])
    one, _ = trx._bar_scene(pkg, "floor", anchors=True, tet=tet)
    one.enable_contact_attribution()
    world = 2
    shards = [trx._bar_scene(pkg, "floor", anchors=True, shard=(r, world), tet=tet)[0] for r in range(world)]
    for sh, hk in zip(shards, _thread_allreduce_hooks(world)):
        sh.set_allreduce(hk)
        sh.enable_contact_attribution()
    pkg.initialize_together(shards)
    assert one.collision_form() == 8 and all(sh.collision_form() == 8 for sh in shards)
    one.step(10)
    out, errs = [None] * world, []

    def run(r):
        try:
            shards[r].step(10)
            out[r] = shards[r].batch_contact_owner(one.coll) + (shards[r].contact_owners(),)
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    ow1, nr1 = one.batch_contact_owner(one.coll)
    ow = np.full(one.N, -9, np.int32); nr = np.full((one.N, 3), np.nan)
    for sh, (o, n_, _) in zip(shards, out):
        loc = sh.local_elements(one.coll)
        assert len(o) == len(loc)
        ow[loc] = o; nr[loc] = n_
    assert np.array_equal(ow, ow1) and np.array_equal(nr, nr1)
    assert (ow1 == 0).sum() >= 4 and (ow1 == -1).sum() >= 4
    assert sorted(np.concatenate([o[2]["node"] for o in out]).tolist()) == one.contact_owners()["node"].tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 10: the C++ class mirror (host/admm/System.hpp): tests/cpp/attribution.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("attribution", pkg))


@pytest.mark.gpu
def test_cpp_mirror_reports_entry_resultants(pkg):
    """Settings::contact_attribution, System::contact_owners and entry_resultants on the scene of tests/cpp/attribution.cpp (refused
    while the switch is off and for a wrong list length: the program checks it) against the same scene built here: the owner records and
    the per-entry resultants bit for bit (%.17g round-trips a double); the floor and the sphere both carry nodes"""
    from test_cpp_host import compile_cpp
    r = subprocess.run([compile_cpp("attribution", pkg)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = {}
    for line in r.stdout.splitlines():
        key, rest = line.split(":", 1)
        vals = []
        for tok in rest.split():
            try:
                vals.append(float(tok))
            except ValueError:
                pass
        rows.setdefault(key, []).append(vals)
    N = 12
    x = np.zeros((N, 3)); v = np.zeros((N, 3))
    for i in range(5):
        x[i] = [0.25 * i, 0.05, 0.125 * i]
        v[i, 1] = -5.0
    for i in range(5, 9):
        x[i] = [5.0 + 0.125 * (i - 6.5), 0.5 + 0.03125 * (i - 5), 0.0625 * (i - 7)]
    for i in range(9, N):
        x[i] = [10.0 + i, 3.0, 0.0]
    s = pkg.System(device_id=0)
    s.set_timestep(0.04)
    s.add_nodes(x.ravel(), np.ones(3 * N))
    s.add_forces(KIND["COLLISION"], np.arange(N, dtype=np.int32), [32.0])
    s.add_gravity([0.0, -9.8, 0.0])
    s.set_collision_shapes([FLOOR, SPHERE], [[0.0, 0.0, 0.0, 0.0], [5.0, 0.2, 0.0, 0.5]])
    s.initialize()
    s.m_v = v.ravel()
    s.step(10)
    s.enable_contact_attribution()
    s.m_x = x.ravel()
    s.m_v = v.ravel()
    s.step(10)
    c, o = s.contacts(), s.contact_owners()
    got = np.array(rows["owner"])
    assert len(got) == len(o) >= 8
    assert np.array_equal(got[:, 0], o["node"]) and np.array_equal(got[:, 1], o["entry"]) and np.array_equal(got[:, 2:5], o["normal"])
    assert np.array_equal(got[:, 5], o["f_normal"]) and np.array_equal(got[:, 6:9], o["f_tangent"]) and np.array_equal(got[:, 9:12], c["f"])
    force, torque, count = s.entry_resultants(pivot=(1.0, 0.0, 0.5))
    want = np.concatenate([np.arange(3)[:, None], count[:, None], force, torque], 1)
    assert np.array_equal(np.array(rows["row"]), want), (rows["row"], want)
    assert count[0] >= 4 and count[1] >= 3
