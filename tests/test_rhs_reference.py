"""The assembled right-hand side of the global step, b = M x_bar + dt^2 D^T W^2 (z - u), against an extended-precision reference.

No other test sees b: it is only visible after A^-1 has been applied.  Here admm_hip_debug_rhs reads the vector the last launch_rhs wrote, and
checkers.RhsReference recomputes it in np.longdouble from the DEVICE's own u and z (read_local) with the oracle's D, W and masses.  Every GPU case:

  1. starts from checkers.deformed_start and runs step(0): the device then holds M x_bar of a known x_bar (m_x after step(0) is x_bar bit for bit);
  2. calls local_step_only twice with two perturbed x_cur (the first leaves a non-zero u, the second is the one checked);
  3. reads u and z back, 4. asserts |debug_rhs() - b_ref| <= bound in EVERY dof, 5. prints the largest ratio.

The bound is derived, not measured (RhsReference's docstring): gamma_k (|m x_bar| + dt^2 |D^T| W^2 |z - u|) per dof with
k = 7 + (T - 1) + (corners on the node - 1): the rounding of fl(z - u_new) (1), of dt^2 w^2 (3), of the two products per term (2), of the T - 1
additions inside a corner, of the at most (corners - 1) additions between the corners of a node whatever the layout, and of the addition of fl(m x_bar) (1).

Sensitivity (CPU arithmetic on the oracle's states, for every GPU scene): removing ONE corner's share moves b_ref by at least 1000 bounds in one
component -- for every corner of each batch's last element (the tail of the last partial block), for every corner on the hub node of the hub meshes,
and for at least 99 % of all corners.  A share that is dropped, duplicated or summed into the wrong slot cannot hide below the bound.

The CPU tie to the oracle (test_reference_reproduces_the_oracle): b_ref from the oracle's own u and z after a one-iteration step, solved with the
oracle's own LDL^T, against the oracle's x_1.  Scale: the relative residual |b - A x|_inf / |b|_inf of that solve (np.longdouble), margin 10 x.
Measured on the 3 x 3 x 7 bar: residual 2.3e-16, |x_ref - x_1|_inf / |x_1|_inf = 4.0e-16, bound 2.3e-15.
"""
import re

import numpy as np
import pytest

from checkers import KIND, KIND_NODES, RhsReference, SparseReference, deformed_start, tet_volumes
from test_residual_reference import LibSim, batch_first, batch_sizes, make_oracle

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).eps > 2.0 ** -63, reason="np.longdouble has no extended precision on this host")
gpu = pytest.mark.gpu
DT = 0.04
GRAVITY = np.array([0.0, -9.8, 0.0])
TET_KINDS = ("TET_LINEAR", "TET_VOLUME", "TET_NH", "TET_STVK")


def _pkg():
    from __graft_entry__ import load_package
    return load_package()


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes: dict(x [n][3], m3 [3n], forces [(kind, idx, params)], start [3n], shapes (types, params) or None, hub: node id or None)
# ---------------------------------------------------------------------------------------------------------------------------------
def bar_scene(dims):
    mg = _pkg().meshgen
    x, t = mg.bar(*dims)
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    forces = [("TET_NH", t, [1e5, 1e5, 5]), ("ANCHOR", mg.bar_anchor_nodes(dims[0], dims[1]), [-1.0, 1.0])]
    return dict(x=x, m3=m3, forces=forces, start=deformed_start(x))


def icosphere(level, radius):
    """-> (vertices [10 4^level + 2][3], triangles [20 4^level][3], oriented outwards)"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(q, dtype=np.float64) / np.sqrt(1.0 + p * p) for q in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = v[a] + v[b]
                v.append(q / np.sqrt(q @ q)); mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return radius * np.array(v), np.array(f, dtype=np.int32)


def hub_scene(level):
    """every triangle of an icosphere joined to ONE hub node at the centre: the hub is a corner of every tet (320 tets on 163 nodes at level 2,
    1280 on 643 at level 3) -- each 64-tet block carries a run of 64 on one node, and the hub has more corners than a block has lanes"""
    v, f = icosphere(level, 0.3)
    x = np.concatenate([v, np.zeros((1, 3))])
    hub = x.shape[0] - 1
    t = np.concatenate([np.full((f.shape[0], 1), hub, np.int32), f], axis=1).astype(np.int32)
    neg = tet_volumes(x, t) < 0
    t[neg] = t[neg][:, [0, 2, 1, 3]]
    assert (tet_volumes(x, t) > 0).all()
    m3 = np.repeat(_pkg().meshgen.lumped_tet_mass(x, t, 1000.0), 3)
    return dict(x=x, m3=m3, forces=[("TET_NH", t, [1e5, 1e5, 5])], start=deformed_start(x), hub=hub)


def mixed_scene():
    """pkg.make_mixed_system(4, 3, 9, 8, 6) restated (NH + StVK tets, cloth triangles, hinges, anchors: the one-launch local step) plus a collision
    batch over all nodes against a floor through the bar (the nodes below it penetrate)"""
    pkg = _pkg(); mg = pkg.meshgen
    x, tets = mg.bar(4, 3, 9)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    half = tets.shape[0] // 2
    xc, tris = mg.sym_plane(8, 6, size=1.0)
    xc = xc + np.array([3.0, 1.0, 0.0])
    off = x.shape[0]
    X = np.concatenate([x, xc]); M = np.concatenate([m, np.full(xc.shape[0], 0.5 / xc.shape[0])])
    n = X.shape[0]
    forces = [("TET_NH", tets[:half], [1e5, 1e5, 5]), ("TET_STVK", tets[half:], [1e5, 1e5, 5]), ("TRI_STRAIN", tris + off, [100.0, 0.95, 1.05, 1.0]),
              ("BEND", mg.bend_hinges(tris) + off, [20.0]),
              ("ANCHOR", np.concatenate([mg.bar_anchor_nodes(4, 3), np.array([off, off + 8], dtype=np.int32)]), [-1.0, 1.0]),
              ("COLLISION", np.arange(n, dtype=np.int32), [32.0])]
    start = deformed_start(X)
    floor_y = 0.06
    assert 0 < (start.reshape(-1, 3)[:, 1] < floor_y).sum() < n
    return dict(x=X, m3=np.repeat(M, 3), forces=forces, start=start, shapes=([0], [[0.0, floor_y, 0.0, 0.0]]))


def test_mixed_scene_is_the_package_s(pkg):
    """the restated scene is make_mixed_system's: same nodes, masses and batches (kinds and sizes) before the collision batch"""
    sc = mixed_scene()
    s, d = pkg.make_mixed_system(4, 3, 9, 8, 6, device_id=-1)
    assert np.array_equal(d["X"], sc["x"]) and np.array_equal(np.repeat(d["M"], 3), sc["m3"])
    assert [(k, np.asarray(i).tolist(), list(p)) for k, i, p in d["forces"]] == [(k, np.asarray(i).tolist(), list(p)) for k, i, p in sc["forces"][:-1]]


SCENES = dict(bar=lambda: bar_scene((5, 4, 11)), hub2=lambda: hub_scene(2), hub3=lambda: hub_scene(3), mixed=mixed_scene, shard_bar=lambda: bar_scene((6, 6, 20)))


def perturbed(xbar):
    """the two x_cur of a case: the first local step leaves a non-zero u behind, the second is the one checked"""
    i = np.arange(xbar.size, dtype=np.float64)
    return xbar + 0.002 * np.sin(1.3 * i), xbar + 0.003 * np.cos(0.7 * i + 0.4)


# ---- the layout rule of upload.inc (upload_all), restated ------------------------------------------------------------------------
def predict_layout(sc, prered=True, tpb=64, node_sorted=False):
    """-> (slots, maxdeg, layout).  A tet batch with pre-reduction leaves one slot per (block, distinct node of the block), blocks of 64 elements
    (`tpb` for the NH / StVK batches); everything else one slot per corner.  Rank-major pads every node to the largest count: used unless that
    more than doubles the array (maxdeg n <= 2 slots + 1024) or ADMM_HIP_SLOTS_NODE_SORTED is set"""
    n = sc["x"].shape[0]
    inc = np.zeros(n, np.int64)
    for kind, idx, par in sc["forces"]:
        idx = np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]])
        if prered and kind in TET_KINDS:
            per = tpb if kind in ("TET_NH", "TET_STVK") else 64
            for b0 in range(0, idx.shape[0], per):
                inc[np.unique(idx[b0:b0 + per])] += 1
        else:
            np.add.at(inc, idx.ravel(), 1)
    slots, maxdeg = int(inc.sum()), int(inc.max())
    return slots, maxdeg, ("rank-major" if maxdeg * n <= 2 * slots + 1024 and not node_sorted else "node-sorted")


def rhs_plan(err):
    """the "plan rhs" lines of ADMM_HIP_VERBOSE (upload.inc) -> [dict(slots, maxdeg, layout, prered)], one per context"""
    return [dict(slots=int(m.group(1)), maxdeg=int(m.group(2)), layout=m.group(3), prered=int(m.group(4)))
            for m in re.finditer(r"admm_hip: plan rhs: slots (\d+) maxdeg (\d+) layout (rank-major|node-sorted) prered ([01])", err)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def oracle_states(sc):
    """the pattern of the GPU cases on the oracle: x_bar of a step with no iteration, then two local steps -> (ref, x_bar, u, z)"""
    o = make_oracle(sc, iters=0)
    ref = RhsReference(o, DT)
    assert o.step()
    xbar = o.x
    assert np.isfinite(xbar).all()
    xa, xb = perturbed(xbar)
    o.local_step(xa, DT)
    u, z = o.local_step(xb, DT)
    assert np.isfinite(u).all() and np.isfinite(z).all()
    return ref, xbar, u, z


def test_reference_reproduces_the_oracle():
    sc = bar_scene((3, 3, 7))
    o = make_oracle(sc, iters=1)
    ref = RhsReference(o, DT)
    x0 = o.x
    xbar = x0 + DT * (np.zeros_like(x0) + np.tile(DT * GRAVITY, x0.size // 3))      # the oracle's own doubles (orc_step: v += (dt g); x + dt v)
    assert o.step()
    x1, u, z = o.x, o.u, o.z
    b = ref.b(xbar, u, z).astype(np.float64)
    xr = o.solve(b)
    A = SparseReference(o, sc["m3"], DT)
    res = float(np.abs(A.residual(xr, b)).max() / np.abs(b).max())
    err = float(np.abs(xr - x1).max() / np.abs(x1).max())
    print("oracle tie: relative residual of the oracle's solve %.3e, |x_ref - x_1| / |x_1| %.3e, bound %.3e" % (res, err, 10 * res))
    assert res > 0 and err <= 10 * res
    # ... and the reference is sensitive in x too: one tet's shares left out move the solution by far more
    drop = ref.corner_force == batch_sizes(sc)[0] - 1
    xd = o.solve(ref.b(xbar, u, z, drop=drop).astype(np.float64))
    assert np.abs(xd - x1).max() / np.abs(x1).max() > 1000 * 10 * res


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_every_share_is_visible(scene):
    sc = SCENES[scene]()
    ref, xbar, u, z = oracle_states(sc)
    sens = ref.corner_sensitivity(xbar, u, z)
    first = batch_first(sc)
    for b, (kind, idx, par) in enumerate(sc["forces"]):
        tail = ref.corner_force == first[b + 1] - 1
        assert tail.sum() == KIND_NODES[KIND[kind]]
        print("%-10s batch %d %-10s last element: weakest corner worth %.2e bounds" % (scene, b, kind, sens[tail].min()))
        assert sens[tail].min() >= 1000, (scene, kind, sens[tail])
    if sc.get("hub") is not None:
        on_hub = ref.corner_node == sc["hub"]
        assert on_hub.sum() == batch_sizes(sc)[0] and ref.degree[sc["hub"]] == on_hub.sum() > 64
        print("%-10s hub: %d corners, the weakest worth %.2e bounds" % (scene, on_hub.sum(), sens[on_hub].min()))
        assert sens[on_hub].min() >= 1000
    frac = float((sens >= 1000).mean())
    print("%-10s %d corners, %.2f %% worth 1000 bounds or more, weakest %.2e, largest k %d" % (scene, sens.size, 100 * frac, sens.min(), ref.k_dof.max()))
    assert frac >= 0.99


def test_layout_rule_on_the_hub_meshes():
    """the oracle initializes on both meshes and stays finite (oracle_states asserts it), and the rule gives the layouts the GPU cases assert"""
    for level, tets, nodes in ((2, 320, 163), (3, 1280, 643)):
        sc = hub_scene(level)
        assert sc["forces"][0][1].shape[0] == tets and sc["x"].shape[0] == nodes
        oracle_states(sc)
    sc2, sc3 = hub_scene(2), hub_scene(3)
    slots, maxdeg, layout = predict_layout(sc2)
    assert (maxdeg, layout) == (5, "rank-major")            # pre-reduced: the hub has one slot per block
    slots, maxdeg, layout = predict_layout(sc2, prered=False)
    assert (slots, maxdeg, layout) == (1280, 320, "node-sorted")      # per corner: 320 slots on the hub, the rule itself leaves rank-major
    slots, maxdeg, layout = predict_layout(sc3)
    assert (maxdeg, layout) == (20, "node-sorted")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def run_case(pkg, name, sc, world=1, mode=None, frames_before=()):
    """-> (the ranks' debug_rhs vectors, the states); asserts the bound in every dof"""
    ref = RhsReference(make_oracle(sc), DT)
    sim = LibSim(pkg, sc, ref, world=world, mode=mode)
    for k in frames_before:
        sim.step(k)
    sim.step(0)
    xbar = sim.state()["x"]
    xa, xb = perturbed(xbar)
    sim._all(lambda s: s.local_step_only(xa))
    sim._all(lambda s: s.local_step_only(xb))
    st = sim.state()
    ys = sim._all(lambda s: s.debug_rhs())
    total = np.zeros(ref.n, np.longdouble)
    for y in ys:
        assert np.isfinite(y).all()
        total = total + y.astype(np.longdouble)
    b_ref, bound = ref.b(xbar, st["u"], st["z"]), ref.bound(xbar, st["u"], st["z"])
    assert (bound > 0).all()
    ratio = np.abs(total - b_ref) / bound
    worst = int(np.argmax(ratio))
    sh = np.abs(ref.shares(st["u"], st["z"])).sum(axis=1)
    first = batch_first(sc)
    for b in range(len(sc["forces"])):      # every batch contributes
        assert sh[(ref.corner_force >= first[b]) & (ref.corner_force < first[b + 1])].sum() > 0, (name, b)
    print("%-44s ranks %d  largest |b_dev - b_ref| / bound %.3f at dof %d (node degree %d, k %d); max |b| %.3e" %
          (name, world, float(ratio[worst]), worst, ref.degree[worst // 3], ref.k_dof[worst], float(np.abs(b_ref).max())))
    assert ratio[worst] <= 1.0, (name, float(ratio[worst]), worst)
    return ys, st, ref


def built(pkg, monkeypatch, capfd, name, sc, env, **kw):
    """run_case under `env` with the plan line read -> (y of the one rank, the plan)"""
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    ys, st, ref = run_case(pkg, name, sc, **kw)
    cap = capfd.readouterr()
    plans = rhs_plan(cap.err)
    with capfd.disabled():      # (the case's own report, which the capture took along)
        print(cap.out, end="")
        print("%-44s plan rhs: %s" % (name, plans))
    assert len(plans) == 1, "no plan rhs line"
    return ys[0], plans[0], ref


def assert_plan(plan, sc, prered=True, tpb=64, node_sorted=False):
    slots, maxdeg, layout = predict_layout(sc, prered, tpb, node_sorted)
    assert plan == dict(slots=slots, maxdeg=maxdeg, layout=layout, prered=int(prered)), (plan, slots, maxdeg, layout)


@pytest.fixture(scope="module")
def bar_default(pkg):
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("ADMM_HIP_DENSE_MAX", "0")
        sc = SCENES["bar"]()
        return sc, run_case(pkg, "bar defaults (shared)", sc)[0][0]
    finally:
        mp.undo()


BAR_KNOBS = [("defaults", {}, {}, True), ("PRERED=0", {"ADMM_HIP_PRERED": "0"}, dict(prered=False), False),
             ("SLOTS_NODE_SORTED=1", {"ADMM_HIP_SLOTS_NODE_SORTED": "1"}, dict(node_sorted=True), True),
             ("TPB=16", {"ADMM_HIP_TPB": "16"}, dict(tpb=16), False),
             ("LOCAL_MULTI=0", {"ADMM_HIP_LOCAL_MULTI": "0"}, {}, True), ("FUSE_ANCHORS=0", {"ADMM_HIP_FUSE_ANCHORS": "0"}, {}, True)]


@gpu
@pytest.mark.parametrize("knob", BAR_KNOBS, ids=[k[0] for k in BAR_KNOBS])
def test_bar_under_each_knob(pkg, monkeypatch, capfd, bar_default, knob):
    """1320 NH tets = 20 full blocks and one of 40, 30 anchors in the tet launch's tail.  The node-sorted layout keeps every node's order (bitwise the
    default), LOCAL_MULTI and FUSE_ANCHORS only change the launch shape (bitwise the default); per-corner slots and 16-tet blocks cut the sums
    elsewhere (the bound only)"""
    name, env, layout, bitwise = knob
    sc, y_default = bar_default
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    assert sc["forces"][0][1].shape[0] == 1320 == 20 * 64 + 40
    y, plan, ref = built(pkg, monkeypatch, capfd, "bar %s" % name, sc, env)
    assert_plan(plan, sc, **layout)
    if name == "PRERED=0":      # rank-major per-corner slots: degrees that run the gather's 8-way unrolled loop AND its remainder
        assert plan["layout"] == "rank-major" and plan["maxdeg"] == ref.degree.max() >= 24
        assert ((ref.degree >= 8) & (ref.degree % 8 != 0)).any() and (ref.degree % 8 == 0).any()
    if name == "SLOTS_NODE_SORTED=1":
        assert plan["layout"] == "node-sorted"
    if name == "defaults":
        assert plan["layout"] == "rank-major"
    if bitwise:
        assert np.array_equal(y, y_default), name


@gpu
def test_bar_layouts_agree_bitwise_without_prereduction(pkg, monkeypatch, capfd):
    """per-corner slots in both layouts: the same per-node order, the same bits"""
    sc = SCENES["bar"]()
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_PRERED", "0")
    ya, pa, _ = built(pkg, monkeypatch, capfd, "bar PRERED=0 rank-major", sc, {})
    yb, pb, _ = built(pkg, monkeypatch, capfd, "bar PRERED=0 node-sorted", sc, {"ADMM_HIP_SLOTS_NODE_SORTED": "1"})
    assert (pa["layout"], pb["layout"]) == ("rank-major", "node-sorted")
    assert np.array_equal(ya, yb)


HUB_CASES = [("hub2", {}, True, "rank-major"), ("hub2", {"ADMM_HIP_PRERED": "0"}, False, "node-sorted"), ("hub3", {}, True, "node-sorted")]


@gpu
@pytest.mark.parametrize("case", HUB_CASES, ids=["level2", "level2-PRERED=0", "level3"])
def test_hub_meshes(pkg, monkeypatch, capfd, case):
    """a node with more corners than a block has lanes, a run of 64 on one node in every block's staging, and the fallback to node-sorted slots
    reached by the RULE (nothing forces it)"""
    scene, env, prered, layout = case
    sc = SCENES[scene]()
    y, plan, ref = built(pkg, monkeypatch, capfd, "%s %s" % (scene, env), sc, env)
    assert_plan(plan, sc, prered=prered)
    assert plan["layout"] == layout
    assert ref.degree[sc["hub"]] == sc["forces"][0][1].shape[0]


@gpu
def test_mixed_scene(pkg, monkeypatch, capfd):
    """six batches (NH, StVK, triangles, hinges, anchors, collisions) in the segments of the one-launch local step share the slot array; one
    launch per batch gives the same bits"""
    sc = SCENES["mixed"]()
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    y1, plan, _ = built(pkg, monkeypatch, capfd, "mixed", sc, {})
    assert_plan(plan, sc)
    y0, plan0, _ = built(pkg, monkeypatch, capfd, "mixed LOCAL_MULTI=0", sc, {"ADMM_HIP_LOCAL_MULTI": "0"})
    assert plan0 == plan
    assert np.array_equal(y0, y1)


@gpu
def test_cost_ordered_launch(pkg, monkeypatch):
    """ADMM_HIP_TET_ORDER_MIN=1: after two frames the blocks start in the order of their cost in the frame before; every block still writes its
    own slots: bitwise what mesh order gives"""
    sc = SCENES["bar"]()
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_TET_ORDER_MIN", "1")
    ya, sta, _ = run_case(pkg, "bar cost order", sc, frames_before=(3, 3))
    monkeypatch.setenv("ADMM_HIP_TET_ORDER", "0")
    yb, stb, _ = run_case(pkg, "bar mesh order", sc, frames_before=(3, 3))
    assert np.array_equal(sta["u"], stb["u"]) and np.array_equal(sta["z"], stb["z"])
    assert np.array_equal(ya[0], yb[0])


@gpu
@pytest.mark.parametrize("world,mode", [(2, "subtree"), (3, "subtree"), (2, "contiguous")])
def test_shards(pkg, monkeypatch, world, mode):
    """every rank assembles its own elements' shares; M x_bar enters exactly once (the base mask under subtree sharding, rank 0 otherwise): the
    long-double sum of the ranks' vectors is b.  A mask that adds M x_bar twice or not at all is off by a whole m x_bar"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    sc = SCENES["shard_bar"]()
    ys, st, ref = run_case(pkg, "6x6x20 bar %s" % mode, sc, world=world, mode=mode)
    # the check is sensitive to the mask: m x_bar of any node is worth far more than the bound there
    mx = np.abs(ref.m3 * st["x"])
    bound = ref.bound(st["x"], st["u"], st["z"]).astype(np.float64).reshape(-1, 3)
    assert ((mx.reshape(-1, 3) / bound).max(axis=1) >= 1000).all()
    assert all(np.abs(y).max() > 0 for y in ys)
