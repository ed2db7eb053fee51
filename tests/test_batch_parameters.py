"""Batches whose elements differ in material, iteration cap and weight.

A batch is a run of consecutive forces of one KIND, not one material: admm_hip_add_batch takes params[n][ADMM_KIND_PARAMS] and
admm::System::initialize merges consecutive same-kind forces whatever their constants.  Every other test hands a batch one parameter
row; here every element has its own (checkers.het_params), so a wrong stride or index into par / kblend / w2 / w2h2 / state, a lane
whose own L-BFGS cap lies below the batch maximum that chose its kernel, or weights rewritten through the wrong element map under
shards give other bits than the oracle, which keeps its parameters per force.

  1. the local step of every kind on 777 disjoint elements, four calls with carried u and warm start: u, z (NH / StVK: warm start and
     iteration counts too) and the weights bit for bit the oracle's.  The hyperelastic kinds twice: caps {1, 3, 5} (the M = 5 kernel) and
     caps {1, 3, 5, 7, 10, 12} (the M = 10 kernel, the history shift beside lanes that never reach it).  CPU: the inputs make every cap
     bind and every cap above 1 be undershot (test_cap_conditions_on_the_oracle; asserted again on the GPU run's oracle counts).
  2. one bar with an NH batch (per-element mu, lambda, cap), anchors with mixed use_weight and springs with per-element stiffness under
     every launch shape that changes how an element finds its data: bitwise the oracle and the default.
  3. the same parameters under 2 / 3 subtree shards and 2 contiguous shards with non-uniform set_weights + recompute_weights.
  4. the class API: consecutive HyperElasticTets of three materials land in ONE batch (tests/cpp/scene_materials.cpp).
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import checkers
from checkers import HYPER_CAPS, HYPER_CAPS_WIDE, KIND, KIND_ROWS, Oracle, het_params
from test_gpu_parity import build_disjoint, disjoint_layout, disjoint_oracle

N = 777                  # ragged against 64 and 256; 13 tet blocks
AMPS = (0.0, 0.02, 0.3, 0.8)
HYPER = ("TET_NH", "TET_STVK")
CASES = [(k, None) for k in ("ANCHOR", "SPRING", "TET_LINEAR", "TET_VOLUME", "TRI_STRAIN", "BEND", "COLLISION", "TRI_AREA", "TRI_FUNG")] + \
        [(k, c) for k in HYPER for c in (HYPER_CAPS, HYPER_CAPS_WIDE)]
SHAPES = ([0, 1, 2], [[0.0, -1.5, 0.0, 0.0], [1.0, 0.5, -0.5, 2.5], [-2.0, 1.0, 0.0, 1.5]])      # floor, sphere, cylinder among the nodes


def case_seed(name, caps):
    return 100 + KIND[name] + len(caps or ())


def case_params(name, caps):
    return het_params(KIND[name], N, np.random.default_rng(1000 + case_seed(name, caps)), caps=caps or HYPER_CAPS)


def calls(X, idx, rng):
    """the four x_cur of test_local_step_bit_exact: amplitudes 0, 0.02, 0.3, 0.8, every seventh element inverted in the last"""
    for it, amp in enumerate(AMPS):
        xcur = (X + amp * rng.normal(size=X.shape)).ravel()
        if it == 3:
            xcur.reshape(-1, 3)[idx[::7, 0]] += 3.0
        yield xcur


def hyper_state(o, f0=0, n=None):
    n = o.n_forces - f0 if n is None else n
    st = np.array([o.hyper_state(f0 + i)[0] for i in range(n)])
    return st, np.array([o.hyper_state(f0 + i)[1] for i in range(n)], np.int32)


def cap_condition(counts, cap, caps):
    """counts [calls][n]: the oracle's L-BFGS iteration counts of every call, cap [n]: every element's own max_iterations.  In at least one
    call EVERY cap value binds (n_iters == cap) on at least three elements; in at least one call every cap above 1 is undershot by at least
    three; with caps above 10, at least three elements of one call run more than 10 iterations (the history shift).  -> the counts."""
    hit = [{c: int(((ni == c) & (cap == c)).sum()) for c in caps} for ni in counts]
    under = [{c: int(((ni < c) & (cap == c)).sum()) for c in caps if c > 1} for ni in counts]
    over10 = [int((ni > 10).sum()) for ni in counts]
    assert all((ni <= cap).all() for ni in counts)
    assert any(min(h.values()) >= 3 for h in hit), hit
    assert any(min(u.values()) >= 3 for u in under), under
    if max(caps) > 10:
        assert max(over10) >= 3, over10
    best = max(range(len(hit)), key=lambda i: min(hit[i].values()))
    return dict(hit=hit[best], under=max(under, key=lambda u: min(u.values())), over10=max(over10))


# ---------------------------------------------------------------- CPU: the conditions on the inputs ----
@pytest.mark.parametrize("caps", [HYPER_CAPS, HYPER_CAPS_WIDE], ids=["caps5", "caps12"])
@pytest.mark.parametrize("name", HYPER)
def test_cap_conditions_on_the_oracle(name, caps):
    """the oracle alone on the inputs of case 1: every cap binds, every cap above 1 is undershot, the wide list shifts its history"""
    P = case_params(name, caps)
    X, idx, rng = disjoint_layout(name, N, case_seed(name, caps))
    o = disjoint_oracle(name, P, X, idx)
    counts = []
    for xcur in calls(X, idx, rng):
        u, z = o.local_step(xcur)
        assert np.isfinite(u).all() and np.isfinite(z).all()
        counts.append(hyper_state(o)[1])
    got = cap_condition(counts, P[:, 2].astype(np.int32), caps)
    print("%s caps %s: %s" % (name, caps, got))


def test_het_params_differ_from_element_to_element():
    """the generator itself: ranges, the integer parameters' value sets, no order in the draws"""
    for name, kind in KIND.items():
        P = het_params(kind, N, np.random.default_rng(kind), caps=HYPER_CAPS_WIDE)
        assert P.shape == (N, checkers.KIND_PARAMS[kind]) and np.isfinite(P).all()
        k = P[:, 0][P[:, 0] > 0]
        assert k.max() / k.min() >= (95.0 if name == "TRI_FUNG" else 100.0), name      # two decades (Fung: [5, 500], the draws' extremes just inside)
        rho = np.corrcoef(np.argsort(np.argsort(P[:, 0])), np.arange(N))[0, 1]
        assert abs(rho) < 0.15, (name, rho)                                        # (3 / sqrt(777) = 0.11)
    P = het_params(KIND["ANCHOR"], N, np.random.default_rng(1))
    assert 0.2 < (P[:, 0] <= 0).mean() < 0.4 and set(P[P[:, 0] <= 0, 0]) == {-1.0, 0.0}
    assert set(het_params(KIND["TRI_AREA"], N, np.random.default_rng(2))[:, 1]) == {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}
    assert set(het_params(KIND["TRI_STRAIN"], N, np.random.default_rng(3))[:, 3]) == {0.0, 1.0}
    assert set(het_params(KIND["TET_STVK"], N, np.random.default_rng(4), caps=HYPER_CAPS_WIDE)[:, 2]) == set(float(c) for c in HYPER_CAPS_WIDE)
    V = het_params(KIND["TET_VOLUME"], N, np.random.default_rng(5))
    assert (V[:, 1] >= 0.7).all() and (V[:, 1] <= 1.0).all() and (V[:, 2] >= 1.0).all() and (V[:, 2] <= 1.3).all()


@pytest.mark.parametrize("name", ["SPRING", "BEND", "ANCHOR", "COLLISION"])
def test_edge_rows_are_present_and_the_oracle_takes_them(name):
    """the inputs test_svd_and_prox_corner_cases_bit_exact adds for the closed-form kinds hold a zero, a denormal, a 1e+-160, an infinite and a
    NaN row, and the oracle's project() of the finite ones stays finite except where a square overflows"""
    import warnings
    kind = KIND[name]; rows = KIND_ROWS[kind]
    Dx, where = checkers.edge_rows(checkers.extreme_matrices(np.random.default_rng(77 + kind), 256), rows)
    assert Dx.shape == (256, rows) and len(set(where.values())) == 8
    x_rest = np.array([0.0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1])
    par = dict(SPRING=[50.0], BEND=[20.0], ANCHOR=[-1.0, 1.0], COLLISION=[32.0])[name]
    Oracle().set_collision_shapes(*SHAPES)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for key in ("zero", "denormal", "tiny"):
            out = Oracle.project_single(kind, x_rest, par, Dx[where[key]])
            assert np.isfinite(out["z"]).all() and np.isfinite(out["u"]).all(), (name, key)
        if name == "SPRING":      # nrm <= 0: the direction is zero, z = c w^2 d = 0 exactly
            assert not Oracle.project_single(kind, x_rest, par, Dx[where["zero"]])["z"].any()
        assert np.isnan(Oracle.project_single(kind, x_rest, par, Dx[where["all_nan"]])["u"]).all()


def test_cpp_materials_program_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_materials", pkg))


# ---------------------------------------------------------------- 1. every kind, bit for bit ----
@pytest.mark.gpu
@pytest.mark.parametrize("name,caps", CASES, ids=["%s%s" % (k, "" if c is None else "-caps%d" % max(c)) for k, c in CASES])
def test_local_step_per_element_parameters_bit_exact(pkg, name, caps):
    P = case_params(name, caps)
    s, o, X, idx, rng = build_disjoint(pkg, name, P, N, seed=case_seed(name, caps))
    if name == "COLLISION":
        s.set_collision_shapes(*SHAPES); o.set_collision_shapes(*SHAPES)
    rows = KIND_ROWS[KIND[name]]
    assert np.array_equal(s.read_rest(0)["weight"], o.weights())      # incl. the fp32 sqrtf path and the anchors' 1000.f default
    if name == "ANCHOR":
        assert 0.2 * N < (o.weights() == 1000.0).sum() < 0.4 * N
    counts = []
    for it, xcur in enumerate(calls(X, idx, rng)):
        s.local_step_only(xcur)
        g = s.read_local(0)
        u, z = (a.reshape(N, rows) for a in o.local_step(xcur))
        if name == "TRI_FUNG":      # sanitised exactly as test_local_step_fung: the tuples the reference itself drives to NaN are skipped
            fin = np.isfinite(z).all(axis=1) & np.isfinite(u).all(axis=1)
            assert fin.sum() > N // 2, (it, int(fin.sum()))
            assert np.array_equal(g["z"][fin], z[fin]) and np.array_equal(g["u"][fin], u[fin]), (name, it)
            st = hyper_state(o)[0]
            u[~fin] = 0.0; st[~np.isfinite(st)] = 1.0
            s.write_local(0, u=u, state=st)
            o._view("u", o.rows)[:] = u.ravel()
            continue
        assert np.array_equal(g["z"], z, equal_nan=True), (name, it, np.flatnonzero((g["z"] != z).any(axis=1))[:8])
        assert np.array_equal(g["u"], u, equal_nan=True), (name, it, np.flatnonzero((g["u"] != u).any(axis=1))[:8])
        if name in HYPER:
            st, ni = hyper_state(o)
            assert np.array_equal(g["n_iters"], ni), (name, it, np.flatnonzero(g["n_iters"] != ni)[:8])
            assert np.array_equal(g["state"], st, equal_nan=True), (name, it)
            counts.append(ni)
    if name in HYPER:
        print("%s caps %s: %s" % (name, caps, cap_condition(counts, P[:, 2].astype(np.int32), caps)))


# ---------------------------------------------------------------- 2. one scene, every launch shape ----
BAR = (6, 5, 17)


def bar_scene(pkg):
    """a 6 x 5 x 17 bar: NH tets with per-element (mu, lambda, cap in {1, 3, 5}) dealt by a seeded permutation, the k = 0 face anchored with
    mixed use_weight, 300 springs of per-element stiffness between random node pairs -> (x, m3, forces, the two x_cur of the local steps)"""
    mg = pkg.meshgen
    rng = np.random.default_rng(2024)
    x, t = mg.bar(*BAR)
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    Pt = het_params(KIND["TET_NH"], t.shape[0], rng)[rng.permutation(t.shape[0])]
    anchors = mg.bar_anchor_nodes(BAR[0], BAR[1])
    a = rng.integers(0, x.shape[0], size=300)
    pairs = np.stack([a, (a + 1 + rng.integers(0, x.shape[0] - 1, size=300)) % x.shape[0]], axis=1).astype(np.int32)
    forces = [("TET_NH", t, Pt), ("ANCHOR", anchors, het_params(KIND["ANCHOR"], anchors.size, rng)), ("SPRING", pairs, het_params(KIND["SPRING"], 300, rng))]
    x0 = checkers.deformed_start(x)
    return x, m3, forces, [x0, x0 + 0.01 * rng.normal(size=x0.size)]


def scene_oracle(x, m3, forces, iters=1):
    o = Oracle(); o.settings(0.04, iters)
    o.add_nodes(np.asarray(x, dtype=np.float64).ravel(), m3)
    for kind, idx, par in forces:
        o.add_forces(KIND[kind], idx, par)
    o.add_gravity([0.0, -9.8, 0.0])
    assert o.initialize()
    return o


def batch_rows(o, forces):
    """per batch: the oracle's rows [n][rows of the kind] of its elements, and its first force"""
    gi, out, f0 = o.global_idx(), [], 0
    for kind, idx, _ in forces:
        n = np.asarray(idx).reshape(-1, checkers.KIND_NODES[KIND[kind]]).shape[0]
        out.append((gi[f0:f0 + n][:, None] + np.arange(KIND_ROWS[KIND[kind]])[None, :], f0))
        f0 += n
    return out


def sync_oracle(o, s, forces):
    """the oracle continues from the device's carried state: u of every batch, the tets' warm start"""
    ou = o._view("u", o.rows)
    for b, (R, f0) in enumerate(batch_rows(o, forces)):
        g = s.read_local(b)
        ou[R] = g["u"]
        if forces[b][0] in HYPER:
            for e in range(R.shape[0]):
                f = o.force(f0 + e)
                for j in range(4):
                    f.state[j] = g["state"][e, j]


def local_steps_vs_oracle(s, o, forces, xcurs, tag):
    """the local steps on the device and the oracle from the same carried state: every batch's u, z (tets: warm start, counts) bit for bit"""
    outs = []
    for c, xcur in enumerate(xcurs):
        s.local_step_only(xcur)
        u, z = o.local_step(xcur)
        for b, (R, f0) in enumerate(batch_rows(o, forces)):
            g = s.read_local(b)
            assert np.array_equal(g["u"], u[R], equal_nan=True) and np.array_equal(g["z"], z[R], equal_nan=True), (tag, c, forces[b][0], np.flatnonzero((g["z"] != z[R]).any(axis=1))[:8])
            if forces[b][0] in HYPER:
                st, ni = hyper_state(o, f0, R.shape[0])
                assert np.array_equal(g["n_iters"], ni) and np.array_equal(g["state"], st, equal_nan=True), (tag, c)
            outs.append(g)
    return outs


def same_outputs(a, b, tag):
    for ga, gb in zip(a, b):
        for k in ("u", "z", "state", "n_iters"):
            assert np.array_equal(ga[k], gb[k], equal_nan=True), (tag, k)


@pytest.fixture(scope="module")
def bar_case(pkg):
    return bar_scene(pkg)


@pytest.fixture(scope="module")
def bar_default(pkg, bar_case):
    """the default launch shape's outputs (the environment as the suite runs it), checked against the oracle once"""
    x, m3, forces, xcurs = bar_case
    s = checkers.scene_system(pkg, x, m3, forces); s.initialize()
    o = scene_oracle(x, m3, forces)
    for b, (R, f0) in enumerate(batch_rows(o, forces)):
        assert np.array_equal(s.read_rest(b)["weight"], o.weights()[f0:f0 + R.shape[0]]), forces[b][0]
    return local_steps_vs_oracle(s, o, forces, xcurs, "default")


@pytest.mark.gpu
@pytest.mark.parametrize("knob,value", [("ADMM_HIP_TPB", "16"), ("ADMM_HIP_LOCAL_MULTI", "0"), ("ADMM_HIP_FUSE_ANCHORS", "0"), ("ADMM_HIP_PRERED", "0"),
                                        ("ADMM_HIP_LOCAL_MULTI+FUSE_ANCHORS", "0")])
def test_launch_shapes_find_every_elements_parameters(pkg, monkeypatch, bar_case, bar_default, knob, value):
    """fewer tets per block, one launch per batch (the anchors as the tet launch's tail, or on their own), per-corner right-hand-side slots:
    the local steps of the per-element bar are bitwise the oracle's and the default's"""
    x, m3, forces, xcurs = bar_case
    for k in knob.replace("+", "+ADMM_HIP_").split("+"):
        monkeypatch.setenv(k, value)
    s = checkers.scene_system(pkg, x, m3, forces); s.initialize()
    same_outputs(local_steps_vs_oracle(s, scene_oracle(x, m3, forces), forces, xcurs, knob), bar_default, knob)


@pytest.mark.gpu
def test_cost_ordered_launch_finds_every_elements_parameters(pkg, monkeypatch, bar_case):
    """ADMM_HIP_TET_ORDER_MIN=8: the 48 tet blocks launch costliest first once a frame has been measured.  Two frames of three iterations
    (per-element caps: the blocks' costs differ), then the local steps from the carried state: frames and local steps bitwise those of the
    mesh-ordered twin, the local steps bitwise the oracle's continued from that state."""
    x, m3, forces, xcurs = bar_case
    outs = []
    for order_min in (None, "8"):
        if order_min:
            monkeypatch.setenv("ADMM_HIP_TET_ORDER_MIN", order_min)
        s = checkers.scene_system(pkg, x, m3, forces); s.initialize()
        s.step(3); s.step(3)
        xf = s.m_x.copy()
        o = scene_oracle(x, m3, forces)
        sync_oracle(o, s, forces)
        outs.append((xf, local_steps_vs_oracle(s, o, forces, xcurs, "order_min %s" % order_min)))
    assert np.isfinite(outs[0][0]).all() and np.array_equal(outs[0][0], outs[1][0])
    same_outputs(outs[0][1], outs[1][1], "cost order")


@pytest.mark.gpu
def test_tracked_kernels_find_every_elements_parameters(pkg, bar_case):
    """enable_residuals: the TRACK instantiations of the tet and anchor kernels, one launch per batch.  u, z, warm start and m_x after
    step(2) are bitwise those of the untracked twin."""
    x, m3, forces, _ = bar_case
    got = []
    for track in (False, True):
        s = checkers.scene_system(pkg, x, m3, forces); s.initialize()
        s.keep_z(True)
        s.enable_residuals(track)
        s.m_x = checkers.deformed_start(x)
        s.step(2)
        got.append((s.m_x.copy(), [s.read_local(b) for b in range(len(forces))]))
    r, sd, n = s.residuals()
    assert n == 2 and np.isfinite(r).all() and (r > 0).all()
    assert np.isfinite(got[0][0]).all() and np.array_equal(got[0][0], got[1][0])
    same_outputs(got[0][1], got[1][1], "tracked")


# ---------------------------------------------------------------- 3. shards ----
SHARD_DIMS = (6, 6, 40)


@pytest.fixture(scope="module")
def shard_case(pkg):
    """the bar of test_knobs.test_sharding_knobs with per-element parameters: the NH scene (local steps against the oracle) and its
    TET_LINEAR twin with per-element stiffness (frames and solves: no truncated minimiser amplifies rounding); seeded weight factors
    in [0.5, 2] for set_weights; the twin's extended-precision reference with those weights"""
    mg = pkg.meshgen
    rng = np.random.default_rng(77)
    x, t = mg.bar(*SHARD_DIMS)
    nt = t.shape[0]
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    anchors = mg.bar_anchor_nodes(SHARD_DIMS[0], SHARD_DIMS[1])
    Pnh = het_params(KIND["TET_NH"], nt, rng)[rng.permutation(nt)]
    Plin = 10.0 ** rng.uniform(2.5, 4.5, size=(nt, 1))
    factor = rng.uniform(0.5, 2.0, size=nt + anchors.size)
    nh = [("TET_NH", t, Pnh), ("ANCHOR", anchors, [-1.0, 1.0])]
    lin = [("TET_LINEAR", t, Plin), ("ANCHOR", anchors, [-1.0, 1.0])]
    ref0 = checkers.scene_reference(x, m3, lin)
    ref = ref0.with_weights(ref0.w0 * factor)
    return dict(x=x, m3=m3, nt=nt, nh=nh, lin=lin, factor=factor, ref=ref, b=rng.normal(size=m3.size))


def shard_systems(pkg, case, forces, world, mode):
    from test_knobs import _bar, _hooks
    ss = [_bar(pkg, forces[0][0], forces[0][2], dims=SHARD_DIMS, rank=r, world=world, mode=mode) for r in range(world)]
    if world > 1:
        hooks = _hooks(world)
        for r, s in enumerate(ss):
            s.set_allreduce(hooks[r])
    pkg.initialize_together(ss, timeout=300.0)
    nt = case["nt"]
    w = np.concatenate([ss[0].read_rest(0)["weight"], ss[0].read_rest(1)["weight"]]) * case["factor"]
    for s in ss:
        s.set_weights(0, w[:nt]); s.set_weights(1, w[nt:])
    pkg.call_together(ss, "recompute_weights", timeout=300.0)
    return ss, w


def together(ss, fn):
    """fn(rank, system) of every rank from its own thread (the calls with an all-reduce inside) -> the results"""
    out, errs = [None] * len(ss), []

    def run(r):
        try:
            out[r] = fn(r, ss[r])
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))
    th = [threading.Thread(target=run, args=(r,)) for r in range(len(ss))]
    [t.start() for t in th]; [t.join(timeout=300) for t in th]
    assert not errs and all(o is not None for o in out), errs
    return out


def frames_and_solve(case):
    def fn(r, s):
        sol = s.solve_only(case["b"])
        xs = []
        for _ in range(2):
            s.step(8); xs.append(s.m_x.copy())
        return sol, xs
    return fn


@pytest.mark.gpu
@pytest.mark.parametrize("world,mode", [(2, "subtree"), (3, "subtree"), (2, "contiguous")])
def test_shards_find_every_elements_parameters_and_weights(pkg, monkeypatch, shard_case, world, mode):
    """per rank, read_local's rows mapped through local_elements are the oracle's u, z and warm start of exactly those elements after
    set_weights + recompute_weights (w2 / w2h2 rewritten through the rank's element map); the ranks end two frames bitwise equal; the
    TET_LINEAR twin agrees with one rank (solve 1e-10 max|x|, frames 1e-9) and the one-rank solve with the extended-precision reference"""
    from test_wide_supernodes import BWD_ERR_TOL, fwd_tol
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    c = shard_case
    nt = c["nt"]
    # -- the NH scene: local steps per rank against the oracle with the same weights
    ss, w = shard_systems(pkg, c, c["nh"], world, mode)
    o = scene_oracle(c["x"], c["m3"], c["nh"])
    assert np.array_equal(w, o.weights() * c["factor"])      # (the device's weights before the edit are the oracle's)
    o.set_weights(w)
    x0 = checkers.deformed_start(c["x"])
    rows = batch_rows(o, c["nh"])
    ids = [[s.local_elements(b) for b in range(2)] for s in ss]
    for b, n in ((0, nt), (1, len(c["nh"][1][1]))):
        cover = np.zeros(n, np.int32)
        for r in range(world):
            cover[ids[r][b]] += 1
        assert (cover >= 1).all(), (b, int((cover == 0).sum()))
    assert all(0 < ids[r][0].size < nt for r in range(world))
    for call, xcur in enumerate((x0, x0 + 0.01 * np.random.default_rng(5).normal(size=x0.size))):
        u, z = o.local_step(xcur)
        st, ni = hyper_state(o, 0, nt)
        for r, s in enumerate(ss):
            s.local_step_only(xcur)
            for b in range(2):
                g, R = s.read_local(b), rows[b][0][ids[r][b]]
                assert np.array_equal(g["u"], u[R]) and np.array_equal(g["z"], z[R]), (call, r, b, np.flatnonzero((g["z"] != z[R]).any(axis=1))[:8])
            g = s.read_local(0)
            assert np.array_equal(g["state"], st[ids[r][0]]) and np.array_equal(g["n_iters"], ni[ids[r][0]]), (call, r)
    out = together(ss, frames_and_solve(c))
    for r in range(1, world):
        assert np.array_equal(out[r][0], out[0][0]) and all(np.array_equal(out[r][1][f], out[0][1][f]) for f in range(2)), r
    assert np.isfinite(out[0][1][1]).all()
    del ss
    # -- the TET_LINEAR twin: ranks bitwise equal, one rank to rounding, one rank against the extended-precision reference
    ss, wl = shard_systems(pkg, c, c["lin"], world, mode)
    one, w1 = shard_systems(pkg, c, c["lin"], 1, None)
    ref = c["ref"]
    assert np.array_equal(wl, w1) and np.array_equal(w1, ref.w0 * c["factor"])
    out = together(ss, frames_and_solve(c))
    sol1, xs1 = frames_and_solve(c)(0, one[0])
    xr, _, _ = ref.solve(c["b"])
    fwd = float(np.abs(sol1 - xr).max() / np.abs(xr).max()); eta = ref.backward_error(sol1, c["b"])
    dsol = max(float(np.abs(out[r][0] - sol1).max() / np.abs(sol1).max()) for r in range(world))
    dfr = max(float(np.abs(out[r][1][f] - xs1[f]).max()) for r in range(world) for f in range(2))
    print("shards %d %s: one-rank forward error / bound %.3g (kappa1 %.3g), backward error / bound %.3g, sharded solve / 1e-10 bound %.3g, frames / 1e-9 bound %.3g"
          % (world, mode, fwd / fwd_tol(ref.kappa1), ref.kappa1, eta / BWD_ERR_TOL, dsol / 1e-10, dfr / 1e-9))
    for r in range(1, world):
        assert np.array_equal(out[r][0], out[0][0]) and all(np.array_equal(out[r][1][f], out[0][1][f]) for f in range(2)), r
    assert fwd <= fwd_tol(ref.kappa1) and eta <= BWD_ERR_TOL
    assert dsol < 1e-10 and dfr < 1e-9


# ---------------------------------------------------------------- 4. the class API ----
@pytest.mark.gpu
def test_class_api_merges_materials_into_one_batch(pkg, tmp_path):
    """tests/cpp/scene_materials.cpp: HyperElasticTets alternating between three (mu, lambda, max_iterations) triples, then Springs of
    per-spring stiffness, then StaticAnchors with mixed use_weight -> three batches; frames bitwise the C ABI's with per-element arrays,
    weights and global_idx the oracle's"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_materials", pkg)
    mg = pkg.meshgen
    rng = np.random.default_rng(31)
    dims = (3, 3, 8)
    x, t = mg.bar(*dims)
    nt = t.shape[0]
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    triples = np.array([[1e5, 1e5, 5.0], [2e3, 4e4, 3.0], [3e4, 1e3, 1.0]])
    a = rng.integers(0, x.shape[0], size=40)
    pairs = np.stack([a, (a + 1 + rng.integers(0, x.shape[0] - 1, size=40)) % x.shape[0]], axis=1).astype(np.int32)
    ks = het_params(KIND["SPRING"], 40, rng)
    anchors = mg.bar_anchor_nodes(dims[0], dims[1])
    pa = het_params(KIND["ANCHOR"], anchors.size, rng)
    frames, iters = 4, 8
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([x.shape[0], nt, 40, anchors.size], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m3.tofile(f); t.astype(np.int32).tofile(f); triples.tofile(f)
        pairs.tofile(f); ks.tofile(f); anchors.astype(np.int32).tofile(f); np.ascontiguousarray(pa[:, 0]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "batches 3: %d x %d, %d x 40, %d x %d" % (KIND["TET_NH"], nt, KIND["SPRING"], KIND["ANCHOR"], anchors.size) in r.stdout, r.stdout
    raw = np.fromfile(outp, dtype=np.float64)
    n3, nf = m3.size, nt + 40 + anchors.size
    XV = raw[:2 * frames * n3].reshape(frames, 2, n3)
    meta = raw[2 * frames * n3:].reshape(nf, 2)
    forces = [("TET_NH", t, triples[np.arange(nt) % 3]), ("SPRING", pairs, ks), ("ANCHOR", anchors, pa)]
    s = checkers.scene_system(pkg, x, m3, forces); s.initialize()
    assert len(s.batches) == 3 and s.info()["n_elems_total"] == nf
    for fr in range(frames):
        s.step(iters)
        assert np.array_equal(XV[fr, 0], s.m_x) and np.array_equal(XV[fr, 1], s.m_v), fr
    assert np.isfinite(XV).all() and np.abs(XV[-1, 0] - x.ravel()).max() > 1e-4
    o = scene_oracle(x, m3, forces, iters)
    assert np.array_equal(meta[:, 1], o.weights())
    assert np.array_equal(meta[:, 0].astype(np.int64), o.global_idx())
    oref = Oracle(ref_layout=True); oref.settings(0.04, iters)
    oref.add_nodes(x.ravel(), m3)
    for kind, idx, par in forces:
        oref.add_forces(KIND[kind], idx, par)
    assert oref.initialize()
    assert np.array_equal(4 * meta[:nt, 0].astype(np.int64), oref.global_idx()[:nt])      # compact rows: the reference's 36 per tet hold 27 zeros
