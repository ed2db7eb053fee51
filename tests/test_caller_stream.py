"""The solver on a caller's non-blocking stream, with skewed queues (GPU).

bench.py and every integration hand the library a torch stream (admm_hip_set_stream); torch's pool streams are created with
hipStreamNonBlocking and have NO implicit ordering with the legacy default stream.  The rest of the suite runs on the stream
admm_hip_create makes with hipStreamCreate, a blocking one, which the runtime serialises against the default stream in both
directions -- so the library's synchronous hipMemcpy / hipMemset calls on the default stream are ordered with its kernels there for
free, and here only where the code says so.

Every case runs a scripted sequence of library calls four times: on the library's own stream (the expected values: what the rest of
the suite pins to the oracle and the reference fixtures; frames are bitwise reproducible) and on the caller's stream

  plain   nothing extra;
  A       a 5-20 ms delay kernel is queued on the CALLER'S stream before every call: the call's own work runs late, so a host read,
          overwrite or free that does not first wait for the context's stream sees the state before the call;
  B       the delay is queued on the LEGACY DEFAULT stream before every call (after initialize: set-up makes dozens of blocking
          uploads): work the library leaves on the default stream runs late, unordered against the kernels on the caller's stream.

Every skewed call is asserted to begin while its delay is still running (checkers.Skew) and counted; every comparison is
np.array_equal.  Two cases also go to references of their own: the local step to the CPU oracle, the solve to the host-assembled A.
Run with -s (or -rP) to see the measured delay and the calls per case.
"""
import gc
import threading
import types

import numpy as np
import pytest

from checkers import HIP_STREAM_NON_BLOCKING, KIND, KIND_ROWS, Delay, Skew, Skewed, nonblocking_stream, same_bits, stream_flags, \
    stream_ordered_allreduce_hooks

pytestmark = pytest.mark.gpu

MODES = ("plain", "A", "B")


@pytest.fixture(scope="module")
def caller():
    """the caller's stream (torch.cuda.Stream, asserted non-blocking), a second one for the second rank, and the calibrated delay"""
    st, flags = nonblocking_stream()
    st2, flags2 = nonblocking_stream()
    assert st2.cuda_stream != st.cuda_stream
    delay = Delay()
    print("caller's stream: hipStreamGetFlags = 0x%x (hipStreamNonBlocking = 0x%x); delay: %s x %d, measured %.2f ms"
          % (flags, HIP_STREAM_NON_BLOCKING, delay.kind, delay.n, delay.ms))
    return types.SimpleNamespace(stream=st, stream2=st2, flags=flags, delay=delay)


def run(pkg, caller, scenario, mode, **kw):
    """scenario(pkg, stream pointer or None, wrap, **kw) -> [(label, value)]; mode "own": the library's stream, unskewed"""
    import torch
    skew = Skew(mode if mode in ("A", "B") else None, caller.stream, caller.delay)

    def wrap(s):
        skew.arm()
        return Skewed(s, skew)
    out = scenario(pkg, None if mode == "own" else caller.stream.cuda_stream, wrap, **kw)
    caller.stream.synchronize(); torch.cuda.default_stream().synchronize()      # delays nobody waited for
    gc.collect()
    if skew.mode:
        assert skew.calls > 0
        print("%s%s, skew %s: %d calls, each begun on a busy queue" % (scenario.__name__, kw or "", mode, skew.calls))
    return out


def check(pkg, caller, scenario, modes=MODES, **kw):
    """the scenario on the library's own stream, then on the caller's under every mode; every mode runs, and every mode's first value
    that differs is named"""
    want = run(pkg, caller, scenario, "own", **kw)
    assert len(want) > 0
    differs = []
    for mode in modes:
        got = run(pkg, caller, scenario, mode, **kw)
        assert [g[0] for g in got] == [w[0] for w in want]
        bad = [(k, w[0]) for k, (w, g) in enumerate(zip(want, got)) if not same_bits(w[1], g[1])]
        if bad:
            differs.append("%s: %d of %d values, the first: value %d (%s)" % (mode, len(bad), len(want), bad[0][0], bad[0][1]))
    assert not differs, "on the caller's stream, against the library's own stream -- " + "; ".join(differs)
    return want


def bar(pkg, dims, ptr, kind="TET_STVK", params=(1e5, 1e5, 5), tip_anchor=False):
    mg = pkg.meshgen
    x, t = mg.bar(*dims)
    m = mg.lumped_tet_mass(x, t, 1000.0)
    s = pkg.System(device_id=0, stream=ptr); s.set_timestep(0.04)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND[kind], t, list(params))
    s.add_forces(KIND["ANCHOR"], mg.bar_anchor_nodes(dims[0], dims[1]), [-1.0, 1.0])
    if tip_anchor:
        tip = x.shape[0] - 1
        s.tip, s.tip_x = s.add_forces(KIND["ANCHOR"], [tip], [-1.0, 1.0], targets=x[tip][None, :]), x[tip].copy()   # a MovingAnchor
    s.add_gravity([0.0, -9.8, 0.0])
    return s


def test_stream_is_non_blocking(caller):
    """the flag as the runtime reports it (hipStreamGetFlags through the HIP runtime the process has loaded) and the delay's length"""
    import torch
    assert caller.flags & HIP_STREAM_NON_BLOCKING and caller.stream.cuda_stream != 0
    assert torch.cuda.default_stream().cuda_stream == 0
    assert 5.0 <= caller.delay.ms <= 20.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. frames and read-backs
# ---------------------------------------------------------------------------------------------------------------------------------
def frames(pkg, ptr, wrap, dense, graph):
    s = bar(pkg, (6, 5, 14), ptr)
    s.initialize()
    assert s.info()["dense_solve"] == (1 if dense else 0)
    s = wrap(s)
    out = []
    reads = [("x", lambda: s.m_x), ("v", lambda: s.m_v), ("tets", lambda: s.read_local(0)), ("anchors", lambda: s.read_local(1))]
    for f, iters in enumerate((10, 10, 10, 10, 7, 1, 10)):
        s.step(iters)
        for k in range(4):      # every read-back is the first one behind a step in some frame: it has to wait for the step itself
            label, read = reads[(f + k) % 4]
            out.append(("%s, frame %d" % (label, f), read()))
        out.append(("graph state, frame %d" % f, s.graph_state()))
        if f == 3:      # graph capture succeeds on the caller's stream as on the library's own
            g = s.graph_state()
            assert g["iter_graph"] == graph and g["frame_graph_iters"] == (10 if graph else 0), g
    return out


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("dense", [False, True])
def test_frames_and_read_backs(pkg, caller, monkeypatch, dense, graph):
    """bar (6, 5, 14), StVK tets + anchors, panel sweeps and the dense default, graph replay and eager launches: step(10) x 4, then
    7, 1, 10 iterations; after every frame m_x, m_v, read_local (u, z, state, n_iters) of both batches and the graph state.
    Shown to fail on two mutants of the library that the own-stream tests cannot see: admm_hip_read_local without its
    hipStreamSynchronize (plain and A: 5 of 35 values, first the tets of frame 2), and the prologue launched on stream 0 (B: 28 of 35
    values, first x of frame 0)."""
    if not dense:
        monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_GRAPH", "1" if graph else "0")
    want = check(pkg, caller, frames, dense=dense, graph=graph)
    xs = [v for label, v in want if label.startswith("x,")]
    assert all(np.isfinite(x).all() for x in xs) and np.abs(xs[-1] - xs[0]).max() > 1e-3      # the bar moves


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. residuals and early exit: the first tracked step allocates and zero-fills the residual buffers inside admm_hip_step
# ---------------------------------------------------------------------------------------------------------------------------------
def residuals(pkg, ptr, wrap):
    s = bar(pkg, (5, 4, 11), ptr)
    s.initialize()
    s = wrap(s)
    s.enable_residuals(True)
    out = []
    for f in range(2):      # (the first of them: ensure_residual_buffers, under the skew)
        s.step(10)
        r, sd, n = s.residuals()
        assert n == 10 and r.size == 10
        out += [("|r|, frame %d" % f, r), ("|s|, frame %d" % f, sd), ("x, frame %d" % f, s.m_x)]
    # a tolerance between two values of the last frame, tested every 2nd iteration; then one every frame meets at its first test
    s.set_tolerance(float(np.sqrt(r[4] * r[5])), float(2.0 * sd.max()), 2)
    s.step(10)
    r2, s2, n2 = s.residuals()
    assert 0 < n2 <= 10 and (n2 == 10 or n2 % 2 == 0)
    out += [("|r|, tolerance", r2), ("|s|, tolerance", s2), ("iterations, tolerance", n2), ("x, tolerance", s.m_x)]
    s.set_tolerance(1e6 * float(r.max()), 1e6 * float(sd.max()), 2)
    s.step(10)
    r3, s3, n3 = s.residuals()
    assert n3 == 2
    out += [("|r|, early exit", r3), ("|s|, early exit", s3), ("iterations, early exit", n3), ("x, early exit", s.m_x), ("v, early exit", s.m_v)]
    return out


@pytest.mark.parametrize("dense", [False, True])
def test_residuals_and_early_exit(pkg, caller, monkeypatch, dense):
    """scene (5, 4, 11): enable_residuals, step(10), residuals(); set_tolerance with check_every = 2: |r|, |s|, the iteration count and m_x"""
    if not dense:
        monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    want = dict(check(pkg, caller, residuals))
    assert (want["|r|, frame 0"] > 0).all() and (want["|s|, frame 0"][1:] > 0).all()
    print("iterations under the tolerance: %d, with the loose one: %d" % (want["iterations, tolerance"], want["iterations, early exit"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. mutators between frames
# ---------------------------------------------------------------------------------------------------------------------------------
def mutators(pkg, ptr, wrap):
    s = bar(pkg, (3, 3, 10), ptr, tip_anchor=True)
    s.initialize()
    tip, tip_x = s.tip, s.tip_x
    s = wrap(s)
    out = []

    def frame(label, iters=10):
        s.step(iters)
        out.append((label, (s.m_x, s.m_v)))
    for f in range(4):      # a moving target, then the release (test_graph_replay_matches_eager_launches), then the re-grab
        s.update_anchors(tip, targets=(tip_x + [0.02 * f, 0.0, 0.0])[None, :], active=[1 if f < 3 else 0])
        frame("anchors %d" % f)
    s.update_anchors(tip, targets=(tip_x + [0.0, 0.03, 0.0])[None, :], active=[1])
    frame("anchors: re-grab")
    s.set_gravity(0, [0.5, -5.0, 1.0])
    frame("gravity")
    s.set_weights(0, s.read_rest(0)["weight"] * 1.5); s.recompute_weights()
    frame("weights")
    out.append(("tets after the new weights", s.read_local(0)))
    r = s.read_local(0)
    s.write_local(0, u=0.5 * r["u"], state=r["state"][::-1].copy())
    out.append(("tets after write_local", s.read_local(0)))
    frame("write_local")
    x, v = s.m_x, s.m_v
    s.m_x = x * (1.0 + 1e-3 * np.sin(np.arange(x.size)))
    s.m_v = 0.5 * v
    out.append(("x, v as set", (s.m_x, s.m_v)))
    frame("setters")
    s.keep_z(False)
    frame("keep_z off"); frame("keep_z off, again")
    s.keep_z(True)
    frame("keep_z on")
    out.append(("tets after keep_z", s.read_local(0)))
    s.enable_timing(True)
    frame("timed")
    t = s.timing()
    assert t["iters"] == 10 and all(np.isfinite(val) and val >= 0.0 for val in t.values()), t
    s.enable_timing(False)
    frame("untimed")
    # the class API's frame boundary: page-locked vectors, then pageable ones
    for pinned in (True, False):
        hx, hv = s.m_x.copy(), s.m_v.copy()
        if pinned:
            s.pin_host(hx); s.pin_host(hv)
        try:
            for f in range(2):
                s.upload_state(hx, hv); s.step(6); s.download_state(hx, hv)
                out.append(("state boundary, %s, frame %d" % ("pinned" if pinned else "pageable", f), (hx.copy(), hv.copy())))
        finally:
            if pinned:
                s.pin_host(hx, False); s.pin_host(hv, False)
    out.append(("x at the end", s.m_x))
    return out


@pytest.mark.parametrize("factor,zerocopy,direct", [("host", "0", "0"), ("device", "1", "0"), ("device", "1", None)])
def test_mutators_between_frames(pkg, caller, monkeypatch, factor, zerocopy, direct):
    """update_anchors (moving target, release, re-grab), set_gravity, set_weights + recompute_weights (host and device
    factorization), write_local, the m_x / m_v setters, keep_z, enable_timing + timing(), upload_state / download_state with
    page-locked and pageable vectors through the zero-copy kernel, the DMA route and the direct route"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    if factor == "host":
        monkeypatch.setenv("ADMM_HIP_FACTOR", "host")
    monkeypatch.setenv("ADMM_HIP_STATE_ZEROCOPY", zerocopy)
    if direct is not None:
        monkeypatch.setenv("ADMM_HIP_STATE_DIRECT", direct)
    want = check(pkg, caller, mutators)
    assert np.isfinite(want[-1][1]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. parity hooks; the local step against the oracle, the solve against the host-assembled matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def parity_hooks(pkg, ptr, wrap):
    s = bar(pkg, (6, 5, 17), ptr)
    s.initialize()
    assert s.info()["device_factor"] == 1 and s.info()["dense_solve"] == 0
    x0 = s.m_x
    s = wrap(s)
    out = []
    rng = np.random.default_rng(17)
    for call, amp in enumerate((0.01, 0.2)):
        s.local_step_only(x0 * (1.0 + amp * np.sin(np.arange(x0.size) * (1.0 + call))))
        out += [("rhs %d" % call, s.debug_rhs()), ("tets %d" % call, s.read_local(0)), ("anchors %d" % call, s.read_local(1))]
    n = s.read_local(0)["u"].shape[0]
    for call in range(2):
        s.local_step_dx(0, (np.eye(3).ravel() + 0.2 * rng.normal(size=(n, 9))))
        out.append(("local_step_dx %d" % call, s.read_local(0)))
    for call in range(2):
        b = rng.normal(size=x0.size)
        sol = s.solve_only(b)
        assert np.abs(s.apply_A(sol) - b).max() < 1e-11 * np.abs(b).max()      # (apply_A: host arithmetic on the assembled A)
        out += [("solve %d" % call, sol), ("host sweeps over the device's factor %d" % call, s.debug_panel_solve_host(b))]
    return out


def test_parity_hooks(pkg, caller, monkeypatch):
    """local_step_only + debug_rhs, local_step_dx, solve_only (every skewed solve within 1e-11 |b| of the host-assembled A, the bound
    of test_knobs.py) and debug_panel_solve_host after a device factorization"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    want = dict(check(pkg, caller, parity_hooks))
    assert np.abs(want["solve 0"] - want["host sweeps over the device's factor 0"]).max() < 1e-10 * np.abs(want["solve 0"]).max()


@pytest.mark.parametrize("mode", ["A", "B"])
def test_local_step_against_the_oracle(pkg, caller, mode):
    """777 disjoint Neo-Hookean tets on the caller's stream under either skew: u, z, the warm start and the L-BFGS iteration counts
    bit for bit the CPU oracle's over the four amplitudes of test_local_step_bit_exact"""
    from test_gpu_parity import build_disjoint, oracle_local_step
    n = 777
    s, o, X, idx, rng = build_disjoint(pkg, "TET_NH", [100.0, 150.0, 5], n, seed=KIND["TET_NH"] + 10)
    s.set_stream(caller.stream.cuda_stream)
    skew = Skew(mode, caller.stream, caller.delay); skew.arm()
    s = Skewed(s, skew)
    rows = KIND_ROWS[KIND["TET_NH"]]
    for it, amp in enumerate((0.0, 0.02, 0.3, 0.8)):
        xcur = (X + amp * rng.normal(size=X.shape)).ravel()
        if it == 3:
            xcur.reshape(-1, 3)[idx[::7, 0]] += 3.0
        s.local_step_only(xcur)
        g = s.read_local(0)
        u, z = oracle_local_step(o, xcur, n, rows)
        st = np.array([o.hyper_state(i)[0] for i in range(n)]); ni = np.array([o.hyper_state(i)[1] for i in range(n)])
        assert np.array_equal(g["z"], z, equal_nan=True) and np.array_equal(g["u"], u, equal_nan=True), (mode, it)
        assert np.array_equal(g["state"], st, equal_nan=True) and np.array_equal(g["n_iters"], ni), (mode, it)
    assert skew.calls == 8
    print("local step against the oracle, skew %s: %d calls, each begun on a busy queue" % (mode, skew.calls))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. collisions
# ---------------------------------------------------------------------------------------------------------------------------------
def collisions(pkg, ptr, wrap):
    """the drop scene of test_collision_shell.py: 65 particles over a floor, a closed cube and an open sheet with side memory"""
    from test_collision_shell import DT, FLOOR, G, IDENT, MESH, R_GPU, W, _cube, _drop_scene, _frame, _grid, _rot
    x = _drop_scene()
    x[:, 1] += 0.25
    Vc, Fc = _cube()
    Vg, Fg = _grid()
    s = pkg.System(device_id=0, stream=ptr)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    cube = s.add_collision_mesh(0.6 * Vc, Fc)
    sheet = s.add_collision_mesh(pkg.Mesh(Vg, Fg, R_GPU), None)
    s.set_collision_mesh_side_memory(sheet, 0.5)
    types, params = [FLOOR, MESH, MESH], [[0, -0.2, 0, 0], [0, 0.0, 0, cube], [0, 0.25, 0, sheet]]
    s.set_collision_shapes(types, params)
    s.initialize()
    assert s.collision_form() == 6
    s = wrap(s)
    out = []

    def frame(label, n=1):
        for _ in range(n):
            s.step(10)
        sides = s.collision_sides(sheet) if len(out) % 2 else None      # (every other time the sides are the first read behind the step)
        out.append((label, (s.m_x, s.m_v, s.collision_sides(sheet) if sides is None else sides)))
    frame("start", 3)
    s.set_collision_friction([0.3, 0.5, 0.2])
    frame("friction", 2)
    s.set_collision_frames([IDENT, _frame(_rot([0.2, 1.0, -0.4], 0.3), [0.0, 0.0, 0.0]), IDENT])
    frame("frames", 2)
    s.set_collision_motion([np.zeros(9), [0.3, 0.0, -0.2, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], np.zeros(9)])
    frame("motion", 2)
    s.update_collision_mesh(cube, 0.6 * Vc * [1.1, 1.0, 0.9])
    bad = 0.6 * Vc.copy(); bad[3, 1] = np.nan
    with pytest.raises(pkg.AdmmHipError) as e:
        s.update_collision_mesh(cube, bad)
    out.append(("the refusal", str(e.value)))
    frame("cube deformed; a refused update", 2)
    s.set_collision_mesh_velocity(cube, np.stack([0.4 * Vc[:, 2], 0.2 + 0.0 * Vc[:, 0], -0.3 * Vc[:, 0]], 1))
    frame("vertex velocities", 2)
    s.set_collision_mesh_thickness(sheet, 0.1875)
    frame("thickness", 2)
    sides = s.collision_sides(sheet)
    s.set_collision_sides(sheet, -sides)
    out.append(("sides as set", s.collision_sides(sheet)))
    s.latch_collision_sides()
    out.append(("sides latched", s.collision_sides(sheet)))
    frame("sides flipped")
    s.reset_collision_sides()
    out.append(("sides after the reset", s.collision_sides(sheet)))
    frame("sides reset", 2)
    s.set_collision_shapes(types[:2], params[:2])
    frame("the sheet taken out of the list", 2)
    return out


def test_collisions(pkg, caller):
    """set_collision_shapes / _friction / _frames / _motion, update_collision_mesh (accepted and refused, the refusal's text the
    same), set_collision_mesh_velocity / _thickness, set_ / latch_ / reset_collision_sides and collision_sides between frames"""
    want = dict(check(pkg, caller, collisions))
    assert "not finite" in want["the refusal"]
    xe = want["the sheet taken out of the list"][0].reshape(-1, 3)
    assert np.isfinite(xe).all() and xe[:, 1].min() > -0.5                  # 20 frames of free fall would end 3.3 lower: the floor held them
    assert (want["start"][2] != 0).any() and (want["sides after the reset"] == 0).all()


def body_surface(pkg, ptr, wrap):
    """the kernel scene of test_body_self_collision.py: the slotted bar closed onto itself, 17 free particles, [floor, body, cube]"""
    from test_body_self_collision import LENGTHS, _kernel_lists, _kernel_scene, _kernel_system
    S, x0, xc, disp = _kernel_scene(pkg)
    entries = _kernel_lists(False)["short"]
    s, b = _kernel_system(pkg, entries, S, x0, LENGTHS)
    if ptr is not None:
        s.set_stream(ptr)
    s = wrap(s)
    rng = np.random.default_rng(173)
    u = np.where((rng.uniform(size=len(x0)) < 0.5)[:, None], 0.0005, 0.002) * rng.normal(size=x0.shape)
    s.m_x = xc.ravel()
    s.write_local(b, u=u)
    s.latch_collision_sides()
    s.local_step_dx(b, xc + disp)
    st = s.body_surface_status(0)
    assert st == dict(updated=1, refused=0, last_bad_tri=-1), st
    out = [("status", st), ("z, u", s.read_local(b))]
    pts = np.concatenate([xc, xc + disp])
    for f in range(2):
        s.step(10)
        m = s.collision_mesh(0)      # (a copy of the surface as the context holds it: its box and its closest points)
        out += [("status %d" % f, s.body_surface_status(0)), ("frame %d" % f, (s.m_x, s.m_v)), ("surface copy %d" % f, (m.info()["lo"], m.info()["hi"], m.closest(pts)))]
    return out


def test_body_surface_status_and_copy(pkg, caller):
    want = dict(check(pkg, caller, body_surface))
    assert want["status 1"]["updated"] + want["status 1"]["refused"] == 3


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. user forces: the pinned staging of D_i x, u, z and the event the host waits on
# ---------------------------------------------------------------------------------------------------------------------------------
def user_forces(pkg, ptr, wrap):
    from test_user_forces import bar_scene, build_system
    scene = bar_scene(pkg)
    s, hook, runs = build_system(pkg, scene)
    if ptr is not None:
        s.set_stream(ptr)
    s.initialize()
    s = wrap(s)
    out = []
    for f in range(6):
        if f == 3:
            s.enable_residuals(True)
        s.step(5)
        first = [s.read_local(b) for b, *_ in runs] if f % 2 else None      # (every other frame the user rows are the first read behind the step)
        out.append(("frame %d" % f, (s.m_x, s.m_v, first or [s.read_local(b) for b, *_ in runs], s.residuals() if f >= 3 else None)))
    out.append(("D_i x as the hook received it", hook.dx))
    assert len(hook.dx) == 6 * 5              # project() once per iteration
    return out


@pytest.mark.parametrize("dense", [False, True])
def test_user_forces(pkg, caller, monkeypatch, dense):
    """bar (3, 3, 10) with Neo-Hookean and volume tets restated as user forces behind a Python project hook: 3 frames with residual
    tracking off and 3 with it on; m_x, m_v, the user rows' u and z, |r|, |s| and every D_i x the hook was handed"""
    if not dense:
        monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    check(pkg, caller, user_forces)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. set_stream mid-life
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "A"])
def test_set_stream_mid_life(pkg, caller, monkeypatch, mode):
    """2 frames on the library's stream (the graphs are captured there), set_stream(torch stream), 2 frames, set_stream(None), 2 frames,
    nothing read back in between: bitwise one uninterrupted own-stream run of 6 frames.  The caller's stream outlives the context.
    (Before admm_hip_set_stream waited for a caller's stream it leaves, both modes failed here: the frames on the new stream ran beside
    the ones still queued on the old.)"""
    import torch
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    ref = bar(pkg, (6, 5, 14), None); ref.initialize()
    for _ in range(6):
        ref.step(10)
    want = (ref.m_x, ref.m_v, ref.read_local(0))
    assert ref.graph_state()["frame_graph_iters"] == 10
    del ref
    skew = Skew("A" if mode == "A" else None, caller.stream, caller.delay)
    raw = bar(pkg, (6, 5, 14), None); raw.initialize()
    s = Skewed(raw, skew)
    s.step(10); s.step(10)
    raw.set_stream(caller.stream.cuda_stream)
    skew.arm()
    s.step(10); s.step(10)
    skew.armed = False
    raw.set_stream(None)
    s.step(10); s.step(10)
    got = (s.m_x, s.m_v, s.read_local(0))
    assert raw.graph_state()["frame_graph_iters"] == 10
    assert same_bits(want, got)
    assert mode != "A" or skew.calls == 2
    del s, raw
    gc.collect()
    with torch.cuda.stream(caller.stream):      # the library has not destroyed the caller's stream
        t = torch.arange(1000, device="cuda", dtype=torch.float64).sum()
    caller.stream.synchronize()
    assert float(t) == 499500.0
    assert stream_flags(caller.stream) & HIP_STREAM_NON_BLOCKING


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. two ranks, each on its own non-blocking stream, behind a hook that relies on stream order alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_ranks(pkg, hooks, streams, skews, b):
    world = 2
    shards = [pkg.make_bar_system(6, 6, 40, kind=KIND["TET_STVK"], rank=r, world=world, shard_mode="subtree",
                                  stream=None if streams is None else streams[r].cuda_stream) for r in range(world)]
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards, timeout=300.0)      # the rank-local factorization's exchange goes through the same hook
    infos = [s.info() for s in shards]
    out, errs = [None] * world, []

    def rank(r):
        try:
            s = shards[r]
            if skews is not None:
                skews[r].arm()
                s = Skewed(s, skews[r])
            xs = []
            for _ in range(2):
                s.step(8)
                xs.append((s.m_x, s.m_v))
            out[r] = (xs, s.solve_only(b))
        except BaseException as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank did not come back"
    assert not errs, errs
    del shards
    gc.collect()
    return out, infos


@pytest.mark.parametrize("mode", ["plain", "A"])
@pytest.mark.parametrize("dist_top", ["0", "1"])
def test_two_ranks_stream_ordered_hook(pkg, caller, monkeypatch, dist_top, mode):
    """bar (6, 6, 40), leaves of 16, two subtree shards on one GPU, each rank in its own thread on its own non-blocking stream; the hook
    records and waits for events and never synchronises the device (checkers.stream_ordered_allreduce_hooks).  initialize_together, 2
    frames of 8 iterations and solve_only, with the replicated and the distributed top: the ranks bitwise equal to each other and to the
    same shards on the library's streams behind the synchronising hook of test_sharding.py"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    monkeypatch.setenv("ADMM_HIP_DIST_TOP", dist_top)
    b = np.random.default_rng(2).normal(size=3 * 7 * 7 * 41)
    want, infos = _two_ranks(pkg, _thread_allreduce_hooks(2), None, None, b)
    assert all(i["dist_top"] == int(dist_top) and i["factor_local"] == 1 and i["nodes_top"] > 0 for i in infos), infos
    assert same_bits(want[0], want[1])
    hooks, calls = stream_ordered_allreduce_hooks(2)
    streams = [caller.stream, caller.stream2]
    skews = [Skew("A" if mode == "A" else None, st, caller.delay) for st in streams]
    got, _ = _two_ranks(pkg, hooks, streams, skews, b)
    assert calls[0] == calls[1] > 2 * 8
    assert same_bits(got[0], got[1]), "the ranks differ from each other behind the stream-ordered hook"
    assert same_bits(got[0], want[0]), "the stream-ordered hook on the callers' streams differs from the synchronising hook"
    if mode == "A":
        assert skews[0].calls == skews[1].calls == 7
        print("two ranks, dist_top %s, skew A: %d calls per rank, each begun on a busy queue; %d hook calls per rank" % (dist_top, skews[0].calls, calls[0]))
