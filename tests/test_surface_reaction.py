"""Two-way contact: the reaction of a contact on the nodes of the body or sheet surface it landed on (System.set_surface_reaction,
admm_hip_set_surface_reaction; csrc/surface_reaction.hpp).

CPU (host-only contexts): surface_reaction_query bit for bit against a plain Python loop that restates the order of the sums, and
against a long-double evaluation within a derived rounding bound; every refusal and the order of the checks.
GPU: the feature's stable sort against numpy's; the device bit for bit against the rule applied from outside by the calls that exist
without it (contacts, contact_owners, collision_mesh, Mesh.closest, mesh_velocity_query -> surface_reaction_query -> m_v) on the two-bar
drop and on a fine block resting on a two-triangle sheet, under every launch mode and solver option; off is off; and the behaviour the
feature exists for: a block dropped on a sheet that has no collision elements of its own now pushes the sheet down."""

import numpy as np
import pytest

from checkers import KIND
from test_body_collision import _two_bars, _with_bodies, _refused, DT, FLOOR_Y, MESH, FLOOR

ADMM_ERR_ARG, ADMM_ERR_HIP, ADMM_ERR_STATE, ADMM_ERR_UNSUPPORTED = 1, 2, 3, 4
U = 2.0 ** -53
REACTING, UNOWNED, OTHER, SELF = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def _restate(m3, f, corner, weight, share, dt):
    """surface_reaction.hpp's order as a plain loop: contacts ascending, corners ascending, one addition per contribution"""
    n = len(m3)
    a = [[0.0, 0.0, 0.0] for _ in range(n)]
    hit = [False] * n
    for k in range(len(f)):
        s = float(share[k])
        if not s > 0.0:
            continue
        p = [float(dt) * float(f[k][j]) for j in range(3)]
        for c in range(3):
            g = s * float(weight[k][c])
            t = int(corner[k][c])
            hit[t] = True
            for j in range(3):
                a[t][j] = a[t][j] + g * p[j]
    dv = np.zeros((n, 3))
    for t in range(n):
        if hit[t]:
            for j in range(3):
                dv[t, j] = a[t][j] / float(m3[t][j])
    return dv, np.array(hit)


def _long_double(m3, f, corner, weight, share, dt):
    """-> (dv in long double, per node and component the sum of |contribution| / m, the number of contributions per node)"""
    L = np.longdouble
    n = len(m3)
    a = np.zeros((n, 3), L); mag = np.zeros((n, 3), L); cnt = np.zeros(n, np.int64)
    for k in range(len(f)):
        if not share[k] > 0.0:
            continue
        for c in range(3):
            t = int(corner[k][c])
            q = L(share[k]) * L(weight[k][c]) * (L(dt) * np.asarray(f[k], L))
            a[t] += q; mag[t] += np.abs(q); cnt[t] += 1
    m = np.asarray(m3, L)
    return a / m, mag / m, cnt


@pytest.mark.parametrize("K", [0, 1, 3, 64, 65, 200])
def test_query_against_restatement_and_long_double(pkg, K):
    """Bitwise against _restate.  Against long double: a contribution q = (s lambda) (dt f) carries three roundings, relative error
    <= 3u + O(u^2), u = 2^-53; the sequential sum of n of them adds at most (n - 1) u times the sum of their magnitudes to first order;
    the division one more u.  So |dv - dv_exact| <= gamma(n + 3) sum |q| / m with gamma(k) = k u / (1 - k u), n the contributions of
    that node; the long-double evaluation's own error (2^-64 per operation) is below u / 1000 of the same magnitude and covered by
    gamma(n + 4).  The destinations are drawn from 3 of 11 nodes and every contact's first corner is node 4, so from K = 65 on that node
    receives more than 64 shares; a tenth of the rows has share 0."""
    rng = np.random.default_rng(100 + K)
    n = 11
    m3 = rng.uniform(0.5, 2.0, (n, 3))
    f = rng.normal(size=(K, 3)) * 10.0 ** rng.integers(-3, 4, (K, 1))
    corner = rng.choice([1, 4, 8], size=(K, 3)).astype(np.int32)
    corner[:, 0] = 4
    w = rng.dirichlet([1.0, 1.0, 1.0], K) if K else np.zeros((0, 3))
    if K:
        w[rng.random(K) < 0.2] = [1.0, 0.0, 0.0]                   # vertex hits
    share = rng.choice([0.25, 0.5, 1.0], K)
    share[rng.permutation(K)[:K // 10]] = 0.0                         # rows with share 0 mixed in
    dt = 0.02
    got = pkg.surface_reaction_query(m3, f, corner, w, share, dt)
    want, hit = _restate(m3, f, corner, w, share, dt)
    assert got.tobytes() == want.tobytes()
    assert np.all(got[~hit] == 0.0) and not np.signbit(got[~hit]).any()
    ref, mag, cnt = _long_double(m3, f, corner, w, share, dt)
    k = (cnt + 4).astype(np.longdouble)[:, None]
    bound = k * U / (1 - k * U) * mag
    err = np.abs(got.astype(np.longdouble) - ref)
    print("K %d: most shares on one node %d, largest error / bound %.3g" % (K, cnt.max() if K else 0, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0))
    assert np.all(err <= bound)
    if K >= 65:
        assert (share == 0).sum() >= 1 and cnt.max() > 64
    # a row with share 0 is not read: corners outside the nodes are fine there, refused where the share is above zero
    if K:
        bad = corner.copy(); bad[0] = [-1, 99, 3]
        s0 = share.copy(); s0[0] = 0.0
        assert pkg.surface_reaction_query(m3, f, bad, w, s0, dt).tobytes() == _restate(m3, f, bad, w, s0, dt)[0].tobytes()
        s0[0] = 0.5
        with pytest.raises(pkg.AdmmHipError):
            pkg.surface_reaction_query(m3, f, bad, w, s0, dt)


def test_query_refusals(pkg):
    m3 = np.ones((4, 3)); f = np.ones((2, 3)); c = np.zeros((2, 3), np.int32); w = np.full((2, 3), 1.0 / 3)
    pkg.surface_reaction_query(m3, f, c, w, 1.0, 0.02)
    for share in (-0.1, 1.5, float("nan")):
        with pytest.raises(pkg.AdmmHipError):
            pkg.surface_reaction_query(m3, f, c, w, share, 0.02)
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.AdmmHipError):
            pkg.surface_reaction_query(m3, f, c, w, 1.0, dt)
    with pytest.raises(pkg.AdmmHipError):
        pkg.surface_reaction_query(np.zeros((0, 3)), f, c, w, 1.0, 0.02)
    one_mass_per_node = pkg.surface_reaction_query(np.ones(4), f, c, w, 1.0, 0.02)
    assert one_mass_per_node.tobytes() == pkg.surface_reaction_query(m3, f, c, w, 1.0, 0.02).tobytes()


def _host_scene(pkg, world=1):
    scene = _two_bars(pkg)
    s = _with_bodies(pkg, scene, device_id=-1, world=world)
    obstacle = s.add_collision_mesh(*_cube(0.1, np.array([2.0, 0.0, 0.0])))
    return s, scene, obstacle


def _cube(h, at):
    v = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], float) * h + at
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, t


def test_refusals_and_order_of_checks(pkg):
    s, scene, obstacle = _host_scene(pkg)
    ia, ib = s.bodies
    # ADMM_ERR_ARG: an unknown mesh, an obstacle, a share outside [0, 1] -- each before the state is looked at (attribution is off)
    _refused(pkg, s, ADMM_ERR_ARG, ["not a registered mesh"], s.set_surface_reaction, 99, 0.5)
    _refused(pkg, s, ADMM_ERR_ARG, ["not a registered mesh"], s.set_surface_reaction, -1, 0.5)
    _refused(pkg, s, ADMM_ERR_ARG, ["obstacle"], s.set_surface_reaction, obstacle, 0.5)
    _refused(pkg, s, ADMM_ERR_ARG, ["obstacle"], s.set_surface_reaction, obstacle, float("nan"))      # the mesh before the share
    for bad in (-0.25, 1.0 + 2.0 ** -52, float("nan"), float("inf")):
        _refused(pkg, s, ADMM_ERR_ARG, ["outside [0, 1]"], s.set_surface_reaction, ia, bad)
    # ADMM_ERR_STATE: a share above zero while contact attribution is off; zero is always fine
    _refused(pkg, s, ADMM_ERR_STATE, ["attribution"], s.set_surface_reaction, ia, 0.5)
    s.set_surface_reaction(ia, 0.0)
    s.enable_contact_attribution(True)
    s.set_surface_reaction(ia, 1.0)
    s.set_surface_reaction(ib, 0.5)
    # ... and the other way round: the switch cannot go off while a share is above zero
    _refused(pkg, s, ADMM_ERR_STATE, ["share"], s.enable_contact_attribution, False)
    s.set_surface_reaction(ia, 0.0)
    _refused(pkg, s, ADMM_ERR_STATE, ["share"], s.enable_contact_attribution, False)
    s.set_surface_reaction(ib, 0.0)
    s.enable_contact_attribution(False)
    s.enable_contact_attribution(True)
    s.set_surface_reaction(ib, 0.5)
    # the depth
    for bad in (-1e-9, float("nan")):
        _refused(pkg, s, ADMM_ERR_ARG, ["depth_min"], s.set_surface_reaction_depth, bad)
    s.set_surface_reaction_depth(0.0)
    s.set_surface_reaction_depth(1e-9)
    # sharding: refused with a share set, in set_shard ...
    _refused(pkg, s, ADMM_ERR_UNSUPPORTED, ["sharded"], s.set_shard, 0, 2)
    s.set_shard(0, 1)
    # the report: its own arguments first, then the host-only context
    _refused(pkg, s, ADMM_ERR_ARG, ["capacity"], s.surface_reaction, -1)
    _refused(pkg, s, ADMM_ERR_HIP, ["host-only"], s.surface_reaction)
    _refused(pkg, s, ADMM_ERR_ARG, ["key_bound"], s.debug_stable_sort, [0, 1], 0)
    _refused(pkg, s, ADMM_ERR_ARG, ["outside"], s.debug_stable_sort, [0, 5], 5)
    _refused(pkg, s, ADMM_ERR_ARG, ["outside"], s.debug_stable_sort, [0, -1], 5)
    _refused(pkg, s, ADMM_ERR_HIP, ["host-only"], s.debug_stable_sort, [0, 1], 5)
    # a host-only context finalizes with shares set, and takes them afterwards too
    s.initialize()
    s.set_surface_reaction(ia, 0.25)
    _refused(pkg, s, ADMM_ERR_STATE, ["share"], s.enable_contact_attribution, False)

    # ... and in set_surface_reaction of a context that is sharded already: ARG before STATE before UNSUPPORTED
    t, _, obstacle = _host_scene(pkg, world=2)
    ia = t.bodies[0]
    _refused(pkg, t, ADMM_ERR_ARG, ["obstacle"], t.set_surface_reaction, obstacle, 0.5)
    _refused(pkg, t, ADMM_ERR_ARG, ["outside [0, 1]"], t.set_surface_reaction, ia, 2.0)
    _refused(pkg, t, ADMM_ERR_STATE, ["attribution"], t.set_surface_reaction, ia, 0.5)
    t.enable_contact_attribution(True)
    _refused(pkg, t, ADMM_ERR_UNSUPPORTED, ["sharded"], t.set_surface_reaction, ia, 0.5)
    t.set_surface_reaction(ia, 0.0)


def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    compile_cpp("surface_reaction", pkg)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorter(pkg):
    s = pkg.make_bar_system(1, 1, 1)
    s.initialize()
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("key_bound", [1, 2, 256, 257, 65537, 2 ** 31 - 1])
def test_stable_sort_against_numpy(pkg, sorter, key_bound):
    """one to four passes (the digits of key_bound - 1); n around the wave width and over many blocks; keys with many duplicates"""
    rng = np.random.default_rng(key_bound % 1000)
    for n in (0, 1, 63, 64, 65, 4097):
        for dup in (False, True):
            if dup:                                                    # a handful of distinct values, the largest key among them
                vals = np.unique(np.concatenate([rng.integers(0, key_bound, 5), [key_bound - 1, 0]]))
                keys = rng.choice(vals, n)
            else:
                keys = rng.integers(0, key_bound, n)
            keys = keys.astype(np.int32)
            got = sorter.debug_stable_sort(keys, key_bound)
            want = np.argsort(keys, kind="stable").astype(np.int32)
            assert np.array_equal(got, want), (key_bound, n, dup)


class _Outside:
    """the rule applied from outside to a context that sets no share: after a step of `s`, from the reports that exist without the
    feature.  surfaces: {mesh_id: (first node, node count, triangles in global node ids)}; types, params: the shape list."""

    def __init__(self, pkg, s, types, params, surfaces, m3, dt, depth_min=0.0):
        self.pkg, self.s, self.types, self.params, self.m3, self.dt, self.depth_min = pkg, s, list(types), np.asarray(params, float).reshape(-1, 4), m3, dt, depth_min
        self.surf = {}
        for mi, (first, count, tris) in surfaces.items():
            self.surf[mi] = (first, count, np.unique(np.asarray(tris).ravel()), s.collision_mesh(mi))

    def apply(self, x0, shares):
        """x0: the positions the frame started from; shares: {mesh_id: share} -> (dv, records, info); writes v - dv into the context"""
        pkg, s = self.pkg, self.s
        c = s.contacts(self.depth_min); o = s.contact_owners(self.depth_min)
        K = len(c)
        assert np.array_equal(c["node"], o["node"])
        rec = np.zeros(K, pkg.SURFACE_CONTACT_DTYPE)
        rec["node"] = c["node"]; rec["mesh"] = -1; rec["tri"] = -1; rec["corner"] = -1
        for k in range(K):
            e = int(o["entry"][k])
            if e < 0:
                rec["status"][k] = UNOWNED
                continue
            mi = int(self.params[e][3]) if self.types[e] == MESH else -1
            rec["mesh"][k] = mi
            if mi not in self.surf or not shares.get(mi, 0.0) > 0.0:
                rec["status"][k] = OTHER
                continue
            first, count = self.surf[mi][:2]
            rec["status"][k] = SELF if first <= c["node"][k] < first + count else REACTING
        for mi, (first, count, nodes, mesh) in self.surf.items():
            rows = np.flatnonzero((rec["status"] == REACTING) & (rec["mesh"] == mi))
            if not len(rows):
                continue
            mesh.set_vertices(x0[nodes])                               # the surface as this frame's start rebuilt it
            e = int(o["entry"][rows[0]])
            t = self.params[e][:3]
            pts = c["point"][rows]
            _, w, ids = pkg.mesh_velocity_query(mesh, None, pts, np.zeros((len(nodes), 3)), t)
            rec["tri"][rows] = mesh.closest(pts - t)["tri"]
            rec["weight"][rows] = w
            rec["corner"][rows] = nodes[ids]
            rec["share"][rows] = shares[mi]
        dv = pkg.surface_reaction_query(self.m3, c["f"], rec["corner"], rec["weight"], rec["share"], self.dt)
        s.m_v = (s.m_v.reshape(-1, 3) - dv).ravel()
        st = rec["status"]
        info = dict(n_contacts=K, n_reacting=int((st == REACTING).sum()), n_unowned=int((st == UNOWNED).sum()), n_other=int((st == OTHER).sum()), n_self=int((st == SELF).sum()))
        return dv, rec, info


def _same_records(a, b):
    return len(a) == len(b) and all(a[n].tobytes() == b[n].tobytes() for n in a.dtype.names)


def _twin(pkg, make, shares_of_frame, frames, iters=10, depth_min=None, check=True):
    """context A with the shares of every frame set on the device, context B with none and the rule applied from outside; -> per frame
    (x, v, dv, records, info) of A after asserting B's are the same bits"""
    a, desc = make(); b, _ = make()
    types, params, surfaces, m3 = desc
    for s in (a, b):
        s.enable_contact_attribution(True)
    first = shares_of_frame(0)
    for mi, sh in first.items():                                       # (before initialize: finalize allocates)
        a.set_surface_reaction(mi, sh)
    a.initialize(); b.initialize()
    if depth_min is not None:
        a.set_surface_reaction_depth(depth_min)
    out = _Outside(pkg, b, types, params, surfaces, m3, DT, 0.0 if depth_min is None else depth_min)
    res = []
    for f in range(frames):
        shares = shares_of_frame(f)
        for mi, sh in shares.items():
            a.set_surface_reaction(mi, sh)
        x0 = b.m_x.reshape(-1, 3).copy()
        a.step(iters); b.step(iters)
        if any(sh > 0.0 for sh in shares.values()):
            dvb, recb, infob = out.apply(x0, shares)
        else:                                                          # all shares zero: the step launches nothing and the report holds nothing
            dvb, recb = np.zeros((a.n_nodes, 3)), np.zeros(0, pkg.SURFACE_CONTACT_DTYPE)
            infob = dict(n_contacts=0, n_reacting=0, n_unowned=0, n_other=0, n_self=0)
        dva, reca, infoa = a.surface_reaction()
        xa, va = a.m_x.copy(), a.m_v.copy()
        if check:
            assert np.array_equal(xa, b.m_x), (f, "x")
            assert infoa == infob, (f, infoa, infob)
            assert _same_records(reca, recb), (f, "records")
            assert dva.tobytes() == dvb.tobytes(), (f, "dv", np.abs(dva - dvb).max())
            assert va.tobytes() == b.m_v.tobytes(), (f, "v")
        res.append((xa, va, dva, reca, infoa))
    return res, a


def _bars(pkg, kind="TET_NH", setup=None):
    scene = _two_bars(pkg)
    x, _, _, m, na, (sa, sb) = scene

    def make():
        s = _with_bodies(pkg, scene, kind=kind)
        if setup:
            setup(s)
        ia, ib = s.bodies
        types, params = [FLOOR, MESH, MESH], [[0, FLOOR_Y, 0, 0], [0, 0, 0, ia], [0, 0, 0, ib]]
        return s, (types, params, {ia: (0, na, sa), ib: (na, len(x) - na, sb)}, np.repeat(m[:, None], 3, 1))
    return make


def _most_contacts_on_one_node(rec):
    r = rec[rec["status"] == REACTING]
    if not len(r):
        return 0
    pairs = np.unique(np.stack([np.repeat(np.arange(len(r)), 3), r["corner"].ravel()], 1), axis=0)      # (contact, node), a node once per contact
    return int(np.bincount(pairs[:, 1]).max())


BAR_FRAMES = 16


@pytest.mark.gpu
def test_twin_two_bars_bit_for_bit(pkg):
    """the two-bar drop of test_body_collision (bars of 3x3x12 and 3x3x8 cells over a floor, both surfaces in the list), shares 1.0 and
    0.5: after every frame x, v, the records and dv of the device equal those of the rule applied from outside, bit for bit.  Some frame
    must have a reacting contact and a node that receives shares from at least two contacts.  Measured on the MI355X over the 16
    frames (the test's printed lines, profiles/surface_reaction/tests_gpu.txt): reacting contacts per frame 0 until frame 6, then 3, 6, 6, 3, 2, 0, 2, 5, 18, 22 (of 3 to 30 contacts); the most contacts
    on one node per frame up to 8."""
    make = _bars(pkg)
    res, a = _twin(pkg, make, lambda f: {0: 1.0, 1: 0.5}, BAR_FRAMES)
    reacting = [r[4]["n_reacting"] for r in res]
    shared = [_most_contacts_on_one_node(r[3]) for r in res]
    print("two bars: reacting contacts per frame %s; most contacts on one node per frame %s; contacts %s" % (reacting, shared, [r[4]["n_contacts"] for r in res]))
    assert max(reacting) > 0 and max(shared) >= 2
    assert any(np.abs(r[2]).max() > 0.0 for r in res)
    # the report with fewer records than contacts: the first ones, the same counts, nothing written beyond them
    K = res[-1][4]["n_contacts"]
    assert K > 3
    for cap in (0, 3, K, K + 5):
        dv2, rec2, info2 = a.surface_reaction(capacity=cap)
        assert info2 == res[-1][4] and dv2.tobytes() == res[-1][2].tobytes()
        assert len(rec2) == min(cap, K) and _same_records(rec2, res[-1][3][:min(cap, K)])
    # two runs of the device give the same bits
    res2, _ = _twin(pkg, make, lambda f: {0: 1.0, 1: 0.5}, 8, check=False)
    for f in range(8):
        assert res[f][0].tobytes() == res2[f][0].tobytes() and res[f][1].tobytes() == res2[f][1].tobytes() and res[f][2].tobytes() == res2[f][2].tobytes()


@pytest.mark.gpu
def test_class_api_reproduces_the_python_frames(pkg, tmp_path):
    """tests/cpp/surface_reaction.cpp: the two bars through the class API (CollisionBody::reaction_share, Settings::contact_attribution,
    System::surface_reaction) give the frames and the dv of the Python run above, bit for bit"""
    import subprocess
    from test_cpp_host import compile_cpp
    exe = compile_cpp("surface_reaction", pkg)
    scene = _two_bars(pkg)
    x, tets, anch, m, na, (sa, sb) = scene
    frames, iters = BAR_FRAMES, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(tets), len(anch), na, len(sa), len(sb)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (tets, anch, sa, sb):
            a.astype(np.int32).tofile(f)
        np.array([FLOOR_Y, DT]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters), "1.0", "0.5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    n3 = len(x) * 3
    got = np.fromfile(outp).reshape(frames, 3 * n3 + 2)
    s, _ = _bars(pkg)()
    s.enable_contact_attribution(True)
    s.initialize()
    s.set_surface_reaction(0, 1.0); s.set_surface_reaction(1, 0.5)
    reacting = 0
    for f in range(frames):
        s.step(iters)
        dv, rec, info = s.surface_reaction()
        assert got[f, :n3].tobytes() == s.m_x.tobytes() and got[f, n3:2 * n3].tobytes() == s.m_v.tobytes(), f
        assert got[f, 2 * n3:3 * n3].tobytes() == dv.ravel().tobytes(), f
        assert (int(got[f, -2]), int(got[f, -1])) == (info["n_contacts"], info["n_reacting"]), f
        reacting += info["n_reacting"]
    assert reacting > 0


def _block_on_sheet(pkg):
    """a fine block (6x2x6 cells of 5 cm: 49 bottom nodes, 147 in three layers) on a sheet surface of four nodes and two triangles in
    the plane y = 0.  The scene as first described -- the block RESTING on the sheet, its 49 bottom nodes in contact -- cannot meet the
    condition set for it, a single run of more than 64 shares: a contact puts at most one share on a given node (its three corners
    are distinct), so 49 contacts put at most 49 on any.  The block and the two-triangle sheet are kept and the number of contacts is
    raised instead: the sheet is a thick shell of half
    thickness 20 cm and the block starts inside it, its layers 8, 13 and 18 cm above the mid-surface: every node of the lower layers
    is in contact, and each contact puts one share on each of the two nodes of the sheet's diagonal.  A soft collision weight (4) and
    heavy sheet nodes (5 kg, on springs) keep the frames gentle.  Collision elements on the block's nodes only."""
    mg = pkg.meshgen
    xb, tb = mg.bar(6, 2, 6)
    xb = xb + np.array([-0.15, 0.08, -0.15])
    nb = len(xb)
    xs = np.array([[-0.4, 0.0, -0.4], [0.4, 0.0, -0.4], [-0.4, 0.0, 0.4], [0.4, 0.0, 0.4]])
    tris = np.array([[0, 2, 1], [1, 2, 3]], np.int32) + nb           # normals up
    x = np.concatenate([xb, xs])
    m = np.concatenate([mg.lumped_tet_mass(xb, tb, 200.0), np.full(4, 5.0)])

    def make():
        s = pkg.System(device_id=0)
        s.set_timestep(DT)
        s.add_nodes(x.ravel(), np.repeat(m, 3))
        s.add_forces(KIND["TET_LINEAR"], tb.astype(np.int32), [2e4])
        s.add_forces(KIND["TRI_STRAIN"], tris, [100.0, 0.95, 1.05, 1.0])
        s.add_forces(KIND["ANCHOR"], np.arange(nb, nb + 4, dtype=np.int32), [50.0, 1.0])
        s.add_forces(KIND["COLLISION"], np.arange(nb, dtype=np.int32), [4.0])
        s.add_gravity([0.0, -9.8, 0.0])
        sheet = s.add_sheet_surface(nb, 4, tris, 0.2)
        s.set_collision_shapes([MESH], [[0, 0, 0, sheet]])
        return s, ([MESH], [[0, 0, 0, sheet]], {sheet: (nb, 4, tris)}, np.repeat(m[:, None], 3, 1))
    return make, nb, m


@pytest.mark.gpu
def test_twin_many_contacts_onto_few_nodes(pkg):
    """3 K shares span several 64-share blocks of the sort and single runs exceed 64 shares; the twin check as above, with a depth
    threshold of 1e-9 m, and the impulse balance  sum_t m_t dv_t = dt sum_k s_k f_k  per component.
    Bound: the left side is sum_t m (a_t / m), a_t the ordered sum of n_t contributions q = (s lambda)(dt f): three roundings per q, at
    most (n_t - 1) u sum |q| from the additions, two more u for the division and the product with m; the right side differs from the
    exact sum of the q by the weights' sum, which tri_weights leaves within 2 u of one.  With N = the longest run:
    |lhs - rhs| <= gamma(N + 8) sum_k s dt |f_k|, gamma(k) = k u / (1 - k u); both sides are evaluated in long double.
    Measured on the MI355X (profiles/surface_reaction/tests_gpu.txt): 137 and 42 reacting contacts in the first two frames (the block then leaves the shell), 411 shares, the
    longest run 137; the balance's largest error is 0.03 of its bound."""
    make, nb, m = _block_on_sheet(pkg)
    frames = 6
    res, a = _twin(pkg, make, lambda f: {0: 1.0}, frames, depth_min=1e-9)
    L = np.longdouble
    worst = 0.0
    longest, most = 0, 0
    c_all = []
    for f, (x, v, dv, rec, info) in enumerate(res):
        r = rec[rec["status"] == REACTING]
        run = int(np.bincount(r["corner"].ravel()).max()) if len(r) else 0
        longest, most = max(longest, run), max(most, 3 * info["n_contacts"])
        c_all.append(info["n_reacting"])
    print("block on sheet: reacting per frame %s, most shares %d, longest run %d" % (c_all, most, longest))
    assert most > 128 and longest > 64
    # the balance on a fresh pair, where the contacts' f of every frame is at hand
    a, desc = make(); a.enable_contact_attribution(True); a.set_surface_reaction(0, 1.0); a.initialize(); a.set_surface_reaction_depth(1e-9)
    mm = np.repeat(m[:, None], 3, 1).astype(L)
    for f in range(frames):
        a.step(10)
        c = a.contacts(1e-9)
        dv, rec, info = a.surface_reaction()
        assert np.array_equal(c["node"], rec["node"])
        lhs = (mm * dv.astype(L)).sum(0)
        sf = rec["share"][:, None].astype(L) * c["f"].astype(L)
        rhs = L(DT) * sf.sum(0)
        r = rec[rec["status"] == REACTING]
        N = int(np.bincount(r["corner"].ravel()).max()) if len(r) else 0
        k = L(N + 8)
        bound = k * U / (1 - k * U) * L(DT) * np.abs(sf).sum(0)
        err = np.abs(lhs - rhs)
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert np.all(err <= bound), (f, err, bound)
    print("impulse balance: largest error / bound %.3g" % worst)


def _plain_frames(s, frames, iters=10):
    out = []
    for f in range(frames):
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


@pytest.mark.gpu
def test_off_is_off(pkg):
    """shares never set, set before initialize and returned to zero, set after initialize (the buffers then exist) and returned to
    zero: the frames of a context that never called, bit for bit; the report then holds nothing"""
    make = _bars(pkg)
    frames = 12
    runs = []
    for how in ("never", "before", "after"):
        s, _ = make()
        s.enable_contact_attribution(True)
        if how == "before":
            s.set_surface_reaction(0, 0.7); s.set_surface_reaction(1, 1.0)
        s.initialize()
        if how == "after":
            s.set_surface_reaction(0, 0.7); s.set_surface_reaction(1, 1.0)
        if how != "never":
            s.set_surface_reaction(0, 0.0); s.set_surface_reaction(1, 0.0)
        runs.append(_plain_frames(s, frames))
        dv, rec, info = s.surface_reaction()
        assert not dv.any() and len(rec) == 0 and info["n_contacts"] == 0
    for r in runs[1:]:
        for f in range(frames):
            assert runs[0][f][0].tobytes() == r[f][0].tobytes() and runs[0][f][1].tobytes() == r[f][1].tobytes(), f
    plain, _ = make()                                                  # ... and attribution itself changes no bits either
    plain.initialize()
    p = _plain_frames(plain, frames)
    for f in range(frames):
        assert runs[0][f][0].tobytes() == p[f][0].tobytes() and runs[0][f][1].tobytes() == p[f][1].tobytes(), f


@pytest.mark.gpu
def test_launch_modes_give_the_same_frames(pkg, monkeypatch):
    make = _bars(pkg)
    frames = 12
    res = {}
    for env in ({"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_GRAPH": "1"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s, _ = make()
        s.enable_contact_attribution(True)
        s.initialize()
        s.set_surface_reaction(0, 1.0); s.set_surface_reaction(1, 0.5)
        out = []
        for f in range(frames):
            s.step(10)
            out.append((s.m_x.copy(), s.m_v.copy(), s.surface_reaction()[0]))
        g = s.graph_state()
        print("launch mode %s: %s" % (env, g))
        if env.get("ADMM_HIP_GRAPH") == "0":
            assert not g["iter_graph"]
        else:
            assert g["iter_graph"]
        res[tuple(env.items())] = out
    keys = list(res)
    assert any(o[2].any() for o in res[keys[0]])
    for k in keys[1:]:
        for f in range(frames):
            assert all(res[keys[0]][f][j].tobytes() == res[k][f][j].tobytes() for j in range(3)), (k, f)


def _opt_residuals(s):
    s.enable_residuals(True)


def _opt_tolerance(s):
    s.set_tolerance(2e-3, 2e-3, 2)


def _opt_anderson(s):
    s.set_acceleration(3)


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["residuals", "tolerance", "anderson", "share_changes"])
def test_options_against_a_twin_under_the_same_option(pkg, option):
    """residual tracking, an exit by tolerance, Anderson acceleration, and shares that change between frames (on, other values, off,
    on again): the device against the rule applied from outside to a context under the same option"""
    setup = dict(residuals=_opt_residuals, tolerance=_opt_tolerance, anderson=_opt_anderson).get(option)
    make = _bars(pkg, setup=setup)
    if option == "share_changes":
        table = [{0: 1.0, 1: 0.5}] * 7 + [{0: 0.25, 1: 1.0}] * 2 + [{0: 0.0, 1: 0.0}] * 2 + [{0: 0.75, 1: 0.0}] * 5
        shares = lambda f: table[f]
    else:
        shares = lambda f: {0: 1.0, 1: 0.5}
    frames = 16 if option == "share_changes" else 14
    res, a = _twin(pkg, make, shares, frames, iters=20 if option == "tolerance" else 10)
    print("%s: reacting per frame %s" % (option, [r[4]["n_reacting"] for r in res]))
    assert max(r[4]["n_reacting"] for r in res) > 0
    if option == "share_changes":
        assert res[9][4]["n_contacts"] == 0 and not res[9][2].any()       # all shares zero: nothing ran
        assert res[10][4]["n_contacts"] == 0 and not res[10][2].any()
        assert max(r[4]["n_reacting"] for r in res[7:9]) > 0              # the second pair of shares ...
        assert max(r[4]["n_reacting"] for r in res[11:]) > 0             # ... and the shares switched on again both reacted


def _sheet_and_block(pkg):
    """a 9x9-node sheet of side 1 m in the plane y = 0, its corners anchored, registered as a sheet surface (half thickness 3 cm) with
    NO collision elements on its own nodes; a block of 2x2x2 cells above its centre with collision elements; gravity on the block's
    nodes alone"""
    mg = pkg.meshgen
    side, nside = 1.0, 9
    g = np.linspace(-0.5, 0.5, nside) * side
    xs = np.array([[g[i], 0.0, g[j]] for j in range(nside) for i in range(nside)])
    tris = []
    for j in range(nside - 1):
        for i in range(nside - 1):
            p = i + nside * j
            tris += [(p, p + nside, p + 1), (p + 1, p + nside, p + nside + 1)]      # normals up
    tris = np.array(tris, np.int32)
    xb, tb = mg.bar(2, 2, 2)
    xb = xb + np.array([-0.05 + 0.013, 0.05, -0.05 + 0.021])
    ns = len(xs)
    x = np.concatenate([xs, xb])
    m = np.concatenate([np.full(ns, 2.0 / ns), mg.lumped_tet_mass(xb, tb, 100.0)])
    corners = np.array([0, nside - 1, nside * (nside - 1), nside * nside - 1], np.int32)
    centre = (nside * nside) // 2

    def make(share):
        s = pkg.System(device_id=0)
        s.set_timestep(DT)
        s.add_nodes(x.ravel(), np.repeat(m, 3))
        s.add_forces(KIND["TRI_STRAIN"], tris, [100.0, 0.95, 1.05, 1.0])
        s.add_forces(KIND["TET_LINEAR"], (tb + ns).astype(np.int32), [2e4])
        s.add_forces(KIND["ANCHOR"], corners, [-1.0, 1.0])
        s.add_forces(KIND["COLLISION"], np.arange(ns, len(x), dtype=np.int32), [32.0])
        s.add_explicit(pkg.EXPLICIT["CONST"], [0.0, -9.8, 0.0], np.arange(ns, len(x), dtype=np.int32))
        sheet = s.add_sheet_surface(0, ns, tris, 0.03)
        s.set_collision_shapes([MESH], [[0, 0, 0, sheet]])
        s.enable_contact_attribution(True)
        s.initialize()
        if share:
            s.set_surface_reaction(sheet, share)
        return s
    return make, xs, ns, centre, side


@pytest.mark.gpu
def test_a_dropped_block_pushes_the_sheet_down(pkg):
    """without shares the sheet feels nothing: its largest displacement d_off over the run is measured here; with share 1 its centre node
    must move down by more than max(1000 d_off, 1e-3 x the sheet's side) within the same frames.  Measured on the MI355X over 30
    frames (profiles/surface_reaction/tests_gpu.txt): d_off 4.7e-15 m, the centre node down by 0.27 m, 101 reacting contacts."""
    make, xs, ns, centre, side = _sheet_and_block(pkg)
    frames = 30
    off, on = make(0.0), make(1.0)
    d_off, down, reacting = 0.0, 0.0, 0
    for f in range(frames):
        off.step(10); on.step(10)
        X0 = off.m_x.reshape(-1, 3)[:ns]
        d_off = max(d_off, float(np.abs(X0 - xs).max()))
        X1 = on.m_x.reshape(-1, 3)
        assert np.isfinite(X1).all()
        down = max(down, float(xs[centre, 1] - X1[centre, 1]))
        reacting += on.surface_reaction()[2]["n_reacting"]
    print("sheet: largest displacement without shares %.3g m; centre node down by %.4g m with share 1; reacting contacts over the run %d" % (d_off, down, reacting))
    assert reacting > 0
    assert down > max(1000.0 * d_off, 1e-3 * side)
