"""The eight collision kernel forms held to each other's bits (csrc/launch.inc collision_form, csrc/kernels_collision.hpp project_collision_*):
one context that set_collision_shapes walks through every form, a ladder of lists L0 .. L7 that each add what their form introduces, and
for every list Lk the same list with a trigger entry Tj appended that nothing reaches, which moves every collision element onto the kernel
of form j > k.

CPU: every list composed on the host from the host twins alone (shape_query, Mesh.query / query_excluding / query_sided / query_self,
mesh_velocity_query and its excluding / self forms, friction_query_moving), with the counts that keep the GPU tests from passing vacuously.
GPU: the base rungs (form k on Lk) bitwise the host composition; the 28 ladder pairs (form j on Lk + Tj bitwise form k on Lk); a context
without meshes against the big one on the analytic entries of L0 .. L3; three frames of step(10) on L3 + Tj for j = 3 .. 7 bitwise equal.

The scene (registered in this order, so that mesh ids never change): 0 a closed icosphere, 1 a closed cube, 2 the surface of a 2 x 2 x 2
tet body, 3 an open grid (a thick shell), 4 the folded strip of test_sheet_self_collision at half size (a self-colliding sheet), 5 an open
grid with side memory, 6 the slotted bar of test_body_self_collision (a self-colliding body), 7 .. 10 the triggers T4 .. T7.  The triggers
of the forms below 4 are entries, not meshes: a sphere at x = 50 with a coefficient (T1), with a rigid motion too (T2), under a frame (T3).
One collision element per free particle (603) and per node of the strip (113), the bar (144) and the tet body (27): 887 elements, fourteen
64-lane blocks with a last one of 55."""
import numpy as np
import pytest

import test_body_self_collision as tb
import test_sheet_self_collision as tsh
from checkers import KIND
from test_collision_friction import CYLINDER, DT, G, W
from test_collision_frames import BOX, IDENT, _frame, _rot, _rotate, _to_local
from test_collision_mesh import FLOOR, MESH, SPHERE, icosphere
from test_collision_shell import _cube, _grid, _same_frames
from test_moving_friction import _np_rigid

ICO, CUBE, TET, SHELL, SHEET, MEM, BODY = range(7)                                       # the mesh ids of the candidates
TRIG_MESH = {4: 7, 5: 8, 6: 9, 7: 10}                                                    # ... and of the triggers T4 .. T7
N_FREE = 603
FAR = 50.0
Z9 = np.zeros(9)

FLOOR_Y = -0.2
SPH_C, SPH_R = np.array([0.6, 0.0, 0.2]), 0.2
CYL_C, CYL_R = np.array([-0.35, 0.0, 0.0]), 0.15
ICO_T, ICO_R = np.array([0.6, 0.15, 0.7]), 0.2
CUBE_T, CUBE_S = np.array([0.15, -0.05, -0.25]), 0.25
TET_O, TET_H = np.array([0.5, -0.15, -0.3]), 0.1
BOX_C, BOX_H = np.array([1.0, 0.0, 0.3]), np.array([0.1, 0.08, 0.12])
SHELL_T, SHELL_S, SHELL_R = np.array([0.15, -0.08, 0.4]), 0.6, 0.05
STRIP_O, STRIP_S = np.array([-0.3, 0.3, 0.05]), 0.5                                      # the strip of test_sheet_self_collision, scaled by a power of two
STRIP_R = STRIP_S * tsh.R_K
MEM_T, MEM_S, MEM_R, MEM_REACH = np.array([0.15, 0.26, 0.4]), 0.9, 0.02, 0.1             # 0.06 above the closed upper arm of the bar, 0.04 below the strip
MU_TET, MU_SHEET, MU_BODY = 0.5, 0.4, 0.25                                               # the body surfaces' own coefficients

F_FLOOR = _frame(_rot([1.0, 0.0, 0.3], 0.05), [0.1, FLOOR_Y, 0.3])
F_CYL = _frame(_rot([0.1, 0.2, 1.0], 0.1), [CYL_C[0], CYL_C[1], 0.4])
F_ICO = _frame(_rot([0.2, 1.0, -0.4], 0.8), ICO_T + [0.02, 0.0, -0.03])
F_BOX = _frame(_rot([0.2, 0.1, 1.0], 0.6), BOX_C)
M_FLOOR = np.array([0.2, 0.0, -0.1, 0, 0, 0, 0, 0, 0])                                   # a conveyor
M_CYL = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 2.5, CYL_C[0], CYL_C[1], 0.0])                # a turn about the cylinder's axis
M_BOX = np.array([0.1, -0.05, 0.1, 0.3, 0.2, -0.3, 1.0, 0.0, 0.3])


def _field(V, a, b):
    return np.stack([a * np.sin(3 * V[:, 1]) + 0.4 * V[:, 2], -0.5 * V[:, 0] * V[:, 2] + b, 0.7 * np.cos(2 * V[:, 0])], 1)      # not rigid


def _entry(ty, par, mu=0.0, frame=None, motion=None, name=None):
    return dict(ty=ty, par=np.asarray(par, dtype=np.float64), mu=mu, frame=IDENT.copy() if frame is None else frame, motion=Z9 if motion is None else motion,
                name=name, mesh=int(par[3]) if ty == MESH else -1)


_SCENE = {}


def _scene(pkg):
    """the geometry, the state every rung starts from and the lists, built once -> dict"""
    if _SCENE:
        return _SCENE
    mg = pkg.meshgen
    rng = np.random.default_rng(181)
    C = _SCENE
    # --- meshes
    Vi, Fi = icosphere(2, ICO_R)
    Vc, Fc = _cube()
    Vg, Fg = _grid()
    Vst, Fst = tsh._strip(pkg, tsh.GAP_K)
    Vst = STRIP_S * Vst + STRIP_O
    S = tb._surface(pkg, (3, 3, 8))
    xt, tets_t = mg.bar(2, 2, 2, TET_H)
    xt = xt + TET_O
    Ft = mg.tet_surface(tets_t)
    V5, F5 = _grid(2)                                                                    # T5: 3 x 3 nodes
    x7, tets7 = mg.bar(1, 1, 1, 0.1)                                                     # T7: one cube of six tets
    # --- nodes: the strip, the bar, the tet body, the free particles, T5's and T7's nodes
    ns, nb, nt = len(Vst), len(S["x"]), len(xt)
    o_b, o_t, o_f = ns, ns + nb, ns + nb + nt
    o_5 = o_f + N_FREE
    o_7 = o_5 + len(V5)
    n = o_7 + len(x7)
    C.update(ns=ns, nb=nb, nt=nt, o_b=o_b, o_t=o_t, o_f=o_f, o_5=o_5, o_7=o_7, n=n, S=S, Fst=Fst, tets_t=tets_t, Ft=Ft, F5=F5, tets7=tets7)
    C["meshes"] = dict(ico=(Vi, Fi), cube=(CUBE_S * Vc, Fc), shell=(SHELL_S * Vg, Fg), mem=(MEM_S * Vg, Fg), t4=_grid(1), t6=_grid(1))
    # --- the free particles' candidates: a cluster at every obstacle, a few anywhere
    def ball(k, c, R, lo, hi):
        d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        return c + R * (1 - rng.uniform(lo, hi, k))[:, None] * d

    def in_box(k, c, h, depth):
        """inside the box |p - c| < h, one coordinate within depth of its face"""
        p = rng.uniform(-1, 1, (k, 3)) * (h - depth)
        a = rng.integers(0, 3, k)
        p[np.arange(k), a] = (h[a] - rng.uniform(0.1, 1.0, k) * depth) * rng.choice([-1.0, 1.0], k)
        return c + p
    cl = []
    cl.append(np.stack([rng.uniform(-0.6, 1.1, 50), FLOOR_Y - rng.uniform(0.002, 0.04, 50), rng.uniform(-0.4, 0.9, 50)], 1))
    cl.append(ball(50, SPH_C, SPH_R, 0.01, 0.2))
    th = rng.uniform(0, 2 * np.pi, 50); rr = CYL_R * (1 - rng.uniform(0.01, 0.25, 50))
    cl.append(np.stack([CYL_C[0] + rr * np.cos(th), CYL_C[1] + rr * np.sin(th), rng.uniform(-0.3, 0.9, 50)], 1))
    cl.append(ball(60, ICO_T, ICO_R, 0.06, 0.3))
    cl.append(in_box(50, CUBE_T, np.full(3, 0.5 * CUBE_S), 0.04))
    cl.append(in_box(40, TET_O + TET_H, np.full(3, TET_H), 0.03))
    pb = in_box(40, np.zeros(3), BOX_H, 0.03)
    cl.append(BOX_C + pb @ F_BOX[:9].reshape(3, 3).T)
    hs = 0.5 * SHELL_S
    cl.append(SHELL_T + np.stack([rng.uniform(-hs, hs, 60), rng.uniform(-0.9, 0.9, 60) * SHELL_R, rng.uniform(-hs, hs, 60)], 1))
    rim = np.stack([hs + rng.uniform(0.1, 0.6, 16) * SHELL_R, rng.uniform(-0.5, 0.5, 16) * SHELL_R, rng.uniform(-hs, hs, 16)], 1)      # beyond an edge of the rim
    rim[8:] = rim[8:, [2, 1, 0]]
    rim[::2, [0, 2]] *= -1.0
    cor = np.stack([hs + rng.uniform(0.1, 0.5, 8) * SHELL_R, rng.uniform(-0.4, 0.4, 8) * SHELL_R, hs + rng.uniform(0.1, 0.5, 8) * SHELL_R], 1)      # beyond a corner
    cor[:, 0] *= np.where(np.arange(8) % 2, 1.0, -1.0); cor[:, 2] *= np.where(np.arange(8) % 4 < 2, 1.0, -1.0)
    cl += [SHELL_T + rim, SHELL_T + cor]
    k = rng.integers(0, ns, 40)
    cl.append(Vst[k] + np.stack([rng.uniform(-0.04, 0.04, 40), rng.uniform(-0.8, 0.8, 40) * STRIP_R, rng.uniform(-0.04, 0.04, 40)], 1))
    hm = 0.5 * MEM_S
    cl.append(MEM_T + np.stack([rng.uniform(-hm, hm, 50), rng.uniform(-0.9, 0.9, 50) * MEM_REACH, rng.uniform(-hm, hm, 50)], 1))
    cl.append(in_box(40, np.array([0.15, 0.05, 0.4]), np.array([0.15, 0.05, 0.4]), 0.02))                                              # inside the bar's lower arm
    free = np.concatenate(cl)
    free = np.concatenate([free, np.stack([rng.uniform(-0.6, 1.1, N_FREE - len(free)), rng.uniform(-0.25, 0.4, N_FREE - len(free)), rng.uniform(-0.4, 0.9, N_FREE - len(free))], 1)])
    assert len(free) == N_FREE
    # --- registered positions, the frame-start state of every rung (the bar closed onto itself), the candidates
    xr = np.concatenate([Vst, S["x"], xt, free, V5 + [FAR, 0.0, 0.0], x7 + [-FAR, 0.0, 0.0]])
    x0 = xr.copy()
    x0[o_b:o_t][tb._upper(S["x"]), 1] -= tb.H
    x0[o_f:o_5] = free + np.where((rng.uniform(size=N_FREE) < 0.5)[:, None], 0.002, 0.02) * rng.normal(size=free.shape)
    v0 = np.zeros_like(x0)
    v0[:o_f] = 0.3 * _field(4 * x0[:o_f], 0.5, 0.2)
    elems = np.arange(o_5, dtype=np.int32)
    disp = np.zeros((o_5, 3))
    up = np.where(Vst[:, 1] < STRIP_O[1] + 0.5 * STRIP_S * tsh.GAP_K, 1.0, -1.0)
    disp[:ns] = 0.005 * rng.normal(size=(ns, 3))
    disp[:ns, 1] += up * rng.uniform(0.0, 0.055, ns)
    disp[o_b:o_t] = rng.uniform(-0.3 * tb.H, 0.3 * tb.H, (nb, 3))
    disp[o_t:o_f] = 0.01 * rng.normal(size=(nt, 3))
    u = np.where((rng.uniform(size=o_5) < 0.5)[:, None], 0.0005, 0.002) * rng.normal(size=(o_5, 3))
    dx = x0[:o_5] + disp
    dx[o_f:] = free - u[o_f:]
    sides0 = rng.integers(-1, 2, n).astype(np.int32)
    C.update(xr=xr, x0=x0, v0=v0, elems=elems, u=u, dx=dx, sides0=sides0)
    C["vel_ico"] = 0.25 * _field(5 * Vi, 0.6, 0.2)
    C["vel_shell"] = _field(3 * SHELL_S * Vg, 0.5, -0.3)
    C["vid_sheet"] = np.concatenate([np.arange(ns), np.full(o_5 - ns, -1)]).astype(np.int32)
    C["vid_body"] = np.full(o_5, -1, np.int32); C["vid_body"][o_b:o_t] = S["vid"]
    # --- the lists
    inf = np.inf
    L0 = [_entry(FLOOR, [0, FLOOR_Y, 0, 0], name="floor"), _entry(SPHERE, [*SPH_C, SPH_R], name="sphere"), _entry(CYLINDER, [*CYL_C, CYL_R], name="cylinder"),
          _entry(MESH, [*ICO_T, ICO], name="icosphere"), _entry(MESH, [*CUBE_T, CUBE], name="cube"), _entry(MESH, [0, 0, 0, TET], name="tet body")]
    L1 = [dict(e, mu=m) for e, m in zip(L0, [0.3, 0.0, 0.7, 0.15, inf, 0.0])]
    L2 = [dict(e) for e in L1]
    L2[0]["motion"], L2[2]["motion"] = M_FLOOR, M_CYL
    L3 = [dict(e) for e in L2] + [_entry(BOX, [*BOX_H, 0], 0.3, F_BOX, M_BOX, "box")]
    L3[0]["frame"], L3[2]["frame"], L3[3]["frame"] = F_FLOOR, F_CYL, F_ICO
    L4 = L3 + [_entry(MESH, [*SHELL_T, SHELL], 0.7, name="shell")]
    L5 = L4 + [_entry(MESH, [0, 0, 0, SHEET], name="sheet")]
    L6 = L5 + [_entry(MESH, [*MEM_T, MEM], 0.15, name="memory shell")]
    L7 = L6 + [_entry(MESH, [0, 0, 0, BODY], name="body")]
    C["lists"] = [L0, L1, L2, L3, L4, L5, L6, L7]
    far = [FAR, 0.0, 0.0, 0.1]
    C["trig"] = {1: _entry(SPHERE, far, 0.3), 2: _entry(SPHERE, far, 0.3, motion=M_BOX), 3: _entry(SPHERE, far, frame=_frame(_rot([0.3, 1.0, 0.2], 0.7), far[:3])),
                 4: _entry(MESH, [FAR, 0, 0, TRIG_MESH[4]]), 5: _entry(MESH, [0, 0, 0, TRIG_MESH[5]]), 6: _entry(MESH, [FAR, 0, 0, TRIG_MESH[6]]),
                 7: _entry(MESH, [0, 0, 0, TRIG_MESH[7]])}
    return C


def _entries(C, k, j):
    return C["lists"][k] + ([C["trig"][j]] if j > k else [])


def _analytic(C, k):
    """the entries of Lk that are not meshes: floor, sphere, cylinder, from L3 on the box"""
    return [e for e in C["lists"][k] if e["ty"] != MESH]


def _system(pkg, C, device_id, gravity=False):
    """the context: every mesh registered before initialize in the fixed order; an empty list until _apply"""
    s = pkg.System(device_id=device_id)
    s.set_timestep(DT)
    s.add_nodes(C["xr"].ravel(), np.ones(3 * C["n"]))
    S, M = C["S"], C["meshes"]
    s.add_forces(KIND["TRI_STRAIN"], C["Fst"], [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["TET_LINEAR"], S["tets"] + C["o_b"], [2e4])
    s.add_forces(KIND["TET_LINEAR"], C["tets_t"] + C["o_t"], [2e4])
    s.add_forces(KIND["TRI_STRAIN"], C["F5"] + C["o_5"], [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["TET_LINEAR"], C["tets7"] + C["o_7"], [2e4])
    s.batch = s.add_forces(KIND["COLLISION"], C["elems"], [W])
    if gravity:
        s.add_gravity([0.0, -G, 0.0])
    ids = [s.add_collision_mesh(*M["ico"]), s.add_collision_mesh(*M["cube"]), s.add_body_surface(C["o_t"], C["nt"], C["Ft"] + C["o_t"]),
           s.add_collision_mesh(pkg.Mesh(*M["shell"], SHELL_R), None), s.add_sheet_surface(0, C["ns"], C["Fst"], STRIP_R, self_collision=True),
           s.add_collision_mesh(pkg.Mesh(*M["mem"], MEM_R), None), s.add_body_surface(C["o_b"], C["nb"], S["F"] + C["o_b"], self_collision=tb.LENGTHS),
           s.add_collision_mesh(pkg.Mesh(*M["t4"], 0.05), None), s.add_sheet_surface(C["o_5"], 9, C["F5"] + C["o_5"], 0.05, self_collision=True),
           s.add_collision_mesh(pkg.Mesh(*M["t6"], 0.05), None),
           s.add_body_surface(C["o_7"], 8, pkg.meshgen.tet_surface(C["tets7"]) + C["o_7"], self_collision=(0.01, 0.02, 0.03))]
    assert ids == list(range(11))
    s.set_collision_mesh_side_memory(MEM, MEM_REACH)
    s.set_collision_mesh_side_memory(TRIG_MESH[6], 0.1)
    s.initialize()
    return s


def _apply(s, C, k, j):
    """list Lk (+ Tj) with what goes with it: a list of another length starts without coefficients, motions and frames, so the list is
    emptied first and everything is set again; the meshes' velocities and the surfaces' coefficients belong to the context, so they are
    set or cleared for every rung"""
    E = _entries(C, k, j)
    s.set_collision_shapes([], np.zeros((0, 4)))
    s.set_collision_shapes([e["ty"] for e in E], [e["par"] for e in E])
    s.set_collision_friction([e["mu"] for e in E])
    s.set_collision_motion([e["motion"] for e in E])
    s.set_collision_frames([e["frame"] for e in E])
    s.set_collision_mesh_velocity(ICO, C["vel_ico"] if k >= 2 else None)
    s.set_collision_mesh_velocity(SHELL, C["vel_shell"] if k >= 4 else None)
    s.set_body_surface_friction(TET, MU_TET if k >= 2 else 0.0)
    s.set_body_surface_friction(SHEET, MU_SHEET if k >= 5 else 0.0)
    s.set_body_surface_friction(BODY, MU_BODY if k >= 7 else 0.0)
    return E


def _host_meshes(pkg, C):
    """the host twins of the candidates' meshes, the body surfaces at the frame-start x (the arithmetic of the device's frame-start update)"""
    if "host" in C:
        return C["host"]
    M, S = C["meshes"], C["S"]
    x0, xr = C["x0"], C["xr"]
    tn = np.unique(C["Ft"])
    loc = np.full(C["nt"], -1, np.int32); loc[tn] = np.arange(len(tn), dtype=np.int32)
    tet = pkg.Mesh(xr[C["o_t"] + tn], loc[C["Ft"]]); tet.set_vertices(x0[C["o_t"] + tn])
    sheet = pkg.Mesh(xr[:C["ns"]], C["Fst"], STRIP_R); sheet.set_vertices(x0[:C["ns"]])
    rest = np.ascontiguousarray(xr[C["o_b"] + S["sv"]])
    body = pkg.Mesh(rest, S["Fl"]); body.set_vertices(x0[C["o_b"] + S["sv"]])
    C["host"] = {ICO: pkg.Mesh(*M["ico"]), CUBE: pkg.Mesh(*M["cube"]), TET: tet, SHELL: pkg.Mesh(*M["shell"], SHELL_R), SHEET: sheet,
                 MEM: pkg.Mesh(*M["mem"], MEM_R), BODY: body, "rest": rest, "tet_nodes": C["o_t"] + tn, "body_nodes": C["o_b"] + S["sv"]}
    return C["host"]


def _host_sides(pkg, C):
    """the latch of the memory shell on the host from the sides every rung installs and the frame-start x"""
    return _host_meshes(pkg, C)[MEM].side_latch(C["x0"], C["sides0"], MEM_REACH, MEM_T)


def _compose(pkg, C, k, sides=None):
    """list Lk on the host in its order, for every collision element -> (z, stats per entry name)"""
    H = _host_meshes(pkg, C)
    el = C["elems"]
    x0, v0 = C["x0"][el], C["v0"]
    p = C["dx"] + C["u"]
    is_tet = (el >= C["o_t"]) & (el < C["o_f"])
    is_bar = (el >= C["o_b"]) & (el < C["o_t"])
    is_sheet = el < C["ns"]
    vid_s, vid_b = C["vid_sheet"], C["vid_body"]
    stats = {}
    for e in C["lists"][k]:
        ty, par, f, mu, mi = e["ty"], e["par"], e["frame"], e["mu"], e["mesh"]
        st = stats.setdefault(e["name"], {})
        framed = not np.array_equal(f, IDENT)
        t = par[:3]
        vi = wts = None
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
            moved = moved.astype(bool)
        elif mi in (ICO, CUBE):
            proj, sd = H[mi].query(p, t, frame=f if framed else None)
            moved = sd > 0
            q = np.where(moved[:, None], proj, p)
            if mi == ICO and k >= 2:                                                     # caller-set vertex velocities, in the mesh's coordinates: turned by R
                vi, wts, _ = pkg.mesh_velocity_query(H[mi], None, _to_local(f, p) if framed else p, C["vel_ico"], t)
                if framed:
                    vi = _rotate(f, vi)
        elif mi == TET:
            proj, sd = H[TET].query(p)
            moved = (sd > 0) & ~is_tet                                                   # its own nodes skip it
            q = np.where(moved[:, None], proj, p)
            mu = MU_TET if k >= 2 else 0.0
            vi = pkg.mesh_velocity_query(H[TET], None, p, v0[H["tet_nodes"]])[0]
        elif mi == SHELL:
            proj, sd = H[SHELL].query(p, t)
            moved = (proj != p).any(1)
            q = np.where(moved[:, None], proj, p)
            vi, wts, _ = pkg.mesh_velocity_query(H[SHELL], None, p, C["vel_shell"], t)
        elif mi == SHEET:
            q, sd, tri = H[SHEET].query_excluding(p, vid_s, t)
            moved = sd > 0
            own = moved & is_sheet
            assert np.array_equal(q[~moved], p[~moved]) and not (C["Fst"][tri[own]] == vid_s[own, None]).any()
            st["own"] = int(own.sum())
            mu = MU_SHEET
            vi, _, ids = H[SHEET].velocity_query_excluding(p, vid_s, v0[:C["ns"]], t)
            assert (ids[moved] >= 0).all()
        elif mi == MEM:
            sd_ = sides[el]
            q, sd, tri, cr = H[MEM].query_sided(p, sd_, MEM_REACH, t)
            moved = (q != p).any(1)
            st["sided"], st["mirrored"] = int((sd_ != 0).sum()), int(((cr != 0) & (sd_ != 0) & moved).sum())
        else:
            assert mi == BODY
            q = p.copy()
            sf = is_bar & (vid_b >= 0)
            qs, sd, tri, cr = H[BODY].query_self(p[sf], vid_b[sf], H["rest"], *tb.LENGTHS)
            mv = (sd > 0) & (tri >= 0)
            assert np.array_equal(qs[~mv], p[sf][~mv])
            q[sf] = qs
            moved = np.zeros(len(p), bool); moved[sf] = mv
            st["crossed"], st["pushed"] = int((cr != 0).sum()), int((mv & (cr == 0)).sum())
            pf, sdf = H[BODY].query(p[~is_bar])
            mf = sdf > 0
            q[~is_bar] = np.where(mf[:, None], pf, p[~is_bar])
            moved[~is_bar] = mf
            mu = MU_BODY
            vel = v0[H["body_nodes"]]
            vi = np.zeros_like(p)
            vi[sf], _, ids = H[BODY].velocity_query_self(p[sf], vid_b[sf], H["rest"], tb.REACH, tb.RHO, vel)
            assert (ids[mv] >= 0).all()
            vi[~is_bar] = pkg.mesh_velocity_query(H[BODY], None, p[~is_bar], vel)[0]
        st["moved"] = int(moved.sum())
        if k >= 1 and mu > 0:
            w = _np_rigid(e["motion"], q)
            if vi is not None:
                w = w + DT * vi
            q2, mode = pkg.friction_query_moving(p, q, x0, w, mu)
            q = np.where(moved[:, None], q2, q)
            st["mu"], st["stick"], st["slip"] = mu, int((mode[moved] == 1).sum()), int((mode[moved] == 2).sum())
            if wts is not None:                                                          # the regions of the hits that took an interpolated velocity
                nz = (wts[moved] != 0).sum(1)
                st["face"], st["edge"], st["vertex"] = int((nz == 3).sum()), int((nz == 2).sum()), int((nz == 1).sum())
        p = q
    return p, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the host composition alone meets the counts; the forms of all 36 rungs on a host-only context
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ladder_counts_on_the_host(pkg):
    """every list composed from the host twins: every entry moves at least 10 candidates; every entry with a finite coefficient has at
    least 10 contacts where the limit mu * depth binds (the rule clamps the tangential part: slip) and at least 10 where it does not
    (stick); with mu = inf the limit cannot bind, so the cube's entry has at least 10 that stick and none that slip.  At least 10 hits on
    the framed icosphere and 10 on the shell take an interpolated velocity; a point inside a convex closed mesh has its closest point
    inside a face, so the icosphere's are face hits, and the shell's cover face, edge and vertex regions (its rim and corners).  At least
    10 own nodes of the sheet are pushed by a triangle outside their 1-ring, at least 10 nodes hold a side on the memory shell and 10 of
    them are mirrored back, at least 10 own surface nodes of the body cross its skin and 10 are pushed from outside."""
    C = _scene(pkg)
    assert len(C["elems"]) == 887 and len(C["elems"]) % 64 and N_FREE % 256
    sides = _host_sides(pkg, C)
    for k in range(8):
        _, stats = _compose(pkg, C, k, sides)
        print("L%d: %s" % (k, stats))
        assert [e["name"] for e in C["lists"][k]] == list(stats)
        for name, st in stats.items():
            assert st["moved"] >= 10, (k, name, st)
            if "mu" in st:
                assert st["stick"] >= 10 and (st["slip"] >= 10 if np.isfinite(st["mu"]) else st["slip"] == 0), (k, name, st)
        assert ("mu" in stats["tet body"]) == (k >= 2) and all(("mu" in stats[nm]) == (k >= 1) for nm in ("floor", "cylinder", "icosphere", "cube"))
        assert "mu" not in stats["sphere"]
        if k >= 3:
            ico = stats["icosphere"]
            assert ico["face"] + ico["edge"] + ico["vertex"] >= 10 and "mu" in stats["box"]
        if k >= 4:
            sh = stats["shell"]
            assert sh["face"] >= 10 and sh["edge"] >= 3 and sh["vertex"] >= 3, sh
        if k >= 5:
            assert stats["sheet"]["own"] >= 10 and "mu" in stats["sheet"]
        if k >= 6:
            assert stats["memory shell"]["sided"] >= 10 and stats["memory shell"]["mirrored"] >= 10 and "mu" in stats["memory shell"]
        if k >= 7:
            assert stats["body"]["crossed"] >= 10 and stats["body"]["pushed"] >= 10 and "mu" in stats["body"]


def test_every_rung_reaches_its_form_on_the_host(pkg):
    """a host-only context walked through all 36 rungs: the form is j for Lk + Tj, and the calls of a rung are accepted in any order of
    rungs (a list of the same length keeps its coefficients, which a body surface's entry refuses)"""
    C = _scene(pkg)
    s = _system(pkg, C, -1)
    for k in list(range(8)) + list(range(7, -1, -1)):
        for j in range(k, 8):
            _apply(s, C, k, j)
            assert s.collision_form() == j, (k, j, s.collision_form())


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the base rungs against the host composition, the ladder, the analytic-only context, whole frames
# ---------------------------------------------------------------------------------------------------------------------------------
_GPU = {}


def _rung(pkg, k, j):
    """-> (z, u) of one local step of the collision batch at form j on list Lk (+ Tj), from the same state every time; run once each"""
    C = _scene(pkg)
    if "s" not in _GPU:
        _GPU["s"] = _system(pkg, C, 0)
    s = _GPU["s"]
    if (k, j) not in _GPU:
        _apply(s, C, k, j)
        assert s.collision_form() == j, (k, j, s.collision_form())
        s.m_x = C["x0"].ravel()
        s.m_v = C["v0"].ravel()
        s.write_local(s.batch, u=C["u"])
        s.set_collision_sides(MEM, C["sides0"])
        s.latch_collision_sides()                                                        # the body surfaces and their vertices' velocities from m_x and m_v, then the sides
        s.local_step_dx(s.batch, C["dx"])
        r = s.read_local(s.batch)
        _GPU[(k, j)] = (r["z"].copy(), r["u"].copy(), s.collision_sides(MEM))
        for mid in (TET, SHEET, BODY):
            assert s.body_surface_status(mid)["refused"] == 0
    return _GPU[(k, j)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(8))
def test_base_rung_equals_host_composition(pkg, k):
    """form k on list Lk: z and u of the 887 elements bitwise the host composition.  L7 has a self-colliding body, a self-colliding
    sheet, a memory shell, a box, rigid motions and caller-set vertex velocities in one list.  The sides read back from the device are the
    host latch's.  Measured on the MI355X: the counts the device's sides give are the host's (printed by the CPU test)."""
    C = _scene(pkg)
    z, u, sides = _rung(pkg, k, k)
    if k >= 6:
        assert np.array_equal(sides, _host_sides(pkg, C))
    want, stats = _compose(pkg, C, k, sides)
    if k >= 6:
        print("L%d on the MI355X: %d nodes hold a side on the memory shell, %d of them mirrored back" % (k, stats["memory shell"]["sided"], stats["memory shell"]["mirrored"]))
        assert stats["memory shell"]["sided"] >= 10 and stats["memory shell"]["mirrored"] >= 10
    assert np.array_equal(z, want), (np.abs(z - want).max(), np.flatnonzero((z != want).any(1)))
    assert np.array_equal(u, C["u"] + (C["dx"] - want))


@pytest.mark.gpu
@pytest.mark.parametrize("k,j", [(k, j) for k in range(8) for j in range(k + 1, 8)])
def test_form_j_gives_form_k_bits(pkg, k, j):
    """list Lk with the trigger Tj, which nothing reaches: the kernel of form j gives the bits of the kernel of form k on Lk"""
    zk, uk, _ = _rung(pkg, k, k)
    zj, uj, _ = _rung(pkg, k, j)
    assert np.array_equal(zj, zk), (np.abs(zj - zk).max(), np.flatnonzero((zj != zk).any(1)))
    assert np.array_equal(uj, uk)


@pytest.mark.gpu
def test_analytic_only_context_gives_the_same_bits(pkg):
    """a context without meshes (project_collision_kernel) against the big one (project_collision_mesh_kernel) on floor, sphere,
    cylinder: the same nodes, elements, candidates and u.  Then the analytic entries of L1, L2 and L3 with their coefficients, motions
    and frames (L3: the box too): form k on both contexts, the MESH = false instantiation of the friction, moving-friction and framed
    kernels against the MESH = true one"""
    C = _scene(pkg)
    _rung(pkg, 0, 0)
    big = _GPU["s"]
    E = C["lists"][0][:3]
    a = pkg.System(device_id=0)
    a.set_timestep(DT)
    a.add_nodes(C["xr"].ravel(), np.ones(3 * C["n"]))
    b = a.add_forces(KIND["COLLISION"], C["elems"], [W])
    a.set_collision_shapes([e["ty"] for e in E], [e["par"] for e in E])
    a.initialize()
    for k in range(4):
        E = _analytic(C, k)
        out = []
        for s, bt in ((a, b), (big, big.batch)):
            s.set_collision_shapes([], np.zeros((0, 4)))
            s.set_collision_shapes([e["ty"] for e in E], [e["par"] for e in E])
            if k >= 1:
                s.set_collision_friction([e["mu"] for e in E])
                s.set_collision_motion([e["motion"] for e in E])
                s.set_collision_frames([e["frame"] for e in E])
            assert s.collision_form() == k, (k, s.collision_form())
            s.m_x = C["x0"].ravel()
            s.write_local(bt, u=C["u"])
            s.local_step_dx(bt, C["dx"])
            r = s.read_local(bt)
            out.append((r["z"].copy(), r["u"].copy()))
        moved = (out[0][0] != C["dx"] + C["u"]).any(1).sum()
        assert moved >= 100, (k, moved)
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), k


@pytest.mark.gpu
def test_frames_agree_across_forms(pkg):
    """five identical contexts with gravity on L3 + Tj, j = 3 .. 7 (j = 3: L3 itself), three frames of step(10) in the default launch
    mode: m_x and m_v bitwise equal across j after every frame, and the frame graph replayed the higher kernels"""
    C = _scene(pkg)
    res = []
    for j in range(3, 8):
        s = _system(pkg, C, 0, gravity=True)
        _apply(s, C, 3, j)
        assert s.collision_form() == j
        s.m_x = C["x0"].ravel()
        s.m_v = C["v0"].ravel()
        fr = []
        for _ in range(3):
            s.step(10)
            fr.append((s.m_x.copy(), s.m_v.copy()))
        assert s.graph_state()["frame_graph_iters"] == 10, (j, s.graph_state())
        res.append(fr)
    for j, fr in zip(range(4, 8), res[1:]):
        assert _same_frames(res[0], fr), j
    assert np.abs(res[0][-1][0] - C["x0"].ravel()).max() > 1e-2
