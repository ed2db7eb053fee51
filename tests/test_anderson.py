"""Anderson acceleration of the ADMM iteration (include/admm_hip.h "Anderson acceleration"; csrc/anderson.hpp, csrc/kernels_anderson.hpp).

CPU: the host twin of the small solve against numpy.longdouble, argument errors, a host-only context.
GPU: off is off; no history, no change; the rule restated in long double from the device's own g and s_out; the lattice converges in
less than half the iterations; the safeguard; reproducibility; checkpoints; the tolerance exit; refusals; the C++ mirror.

The state s = (z, u) is handled here as one flat vector: batch after batch, the batch's z [n][rows] then its u, with the weights w^2
of the batch's elements repeated over the rows.  Sums do not depend on that order; elementwise checks do not either.
"""
import subprocess

import numpy as np
import pytest

from anderson_cases import (DT, LD, U, _frame_start_z, _pkg, _same_bits, build_system, check_log_invariants, check_rule_restated, checkpoint,
                            flat_state, flat_weights, full_state, lattice_scene, needs_ld, restore)
from checkers import KIND

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the host twin
# ---------------------------------------------------------------------------------------------------------------------------------
# The bound of the issue: the residual of the regularised system, |b - (A + lambda I) theta| <= c m^2 2^-53 |A|_2 |theta|_2.
# c from the operation count: a Cholesky solve gives (A' + dA) theta = b with |dA| <= gamma_(3m+1) |L| |L^T| (Higham, Accuracy and
# Stability, Theorem 10.4) and | |L| |L^T| |_2 <= m |A'|_2 (ibid. (10.7)): m (3m + 1) <= 4 m^2; forming A' = A + lambda I rounds every
# diagonal entry once (<= 2^-53 |A'|_2, less than another m^2 term), and lambda itself carries (m + 1) roundings of a number that is
# 1e-12 |A|: nothing.  c = 5.
C_SOLVE = 5.0


def _gram(cols, w2):
    """the Gram matrix and right-hand side of difference columns [n][m] against f [n], in long double, rounded to double"""
    dF, f = cols
    A = (dF.astype(LD).T * w2.astype(LD)) @ dF.astype(LD)
    b = (dF.astype(LD).T * w2.astype(LD)) @ f.astype(LD)
    return np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)


def _solve_residual(A, b, th):
    """|b - (A + lambda I) theta|_2 in long double and the bound's |A|_2 |theta|_2"""
    m = b.size
    Al = A.astype(LD)
    lam = LD(1e-12) * np.trace(Al) / LD(m)
    r = b.astype(LD) - (Al + lam * np.eye(m, dtype=LD)) @ th.astype(LD)
    return float(np.sqrt(np.sum(r * r))), float(np.linalg.norm(A, 2)) * float(np.linalg.norm(th))


@needs_ld
@pytest.mark.parametrize("mk", range(1, 9))
@pytest.mark.parametrize("case", ["random", "dependent"])
def test_host_twin_against_long_double(mk, case):
    pkg = _pkg()
    rng = np.random.default_rng(100 * mk + (case == "dependent"))
    for trial in range(20):
        n = 200
        dF = rng.normal(size=(n, mk)) * 10.0 ** rng.uniform(-6, 2)
        if case == "dependent" and mk >= 2:      # two columns that differ by 1e-9 relative
            dF[:, 1] = dF[:, 0] * (1.0 + 1e-9 * rng.normal(size=n))
        f = rng.normal(size=n)
        w2 = rng.uniform(0.5, 2000.0, size=n)
        A, b = _gram((dF, f), w2)
        A = np.tril(A) + np.tril(A, -1).T
        th = pkg.acceleration_query(A, b)
        res, scale = _solve_residual(A, b, th)
        assert np.isfinite(th).all() and (th != 0.0).any()
        assert res <= C_SOLVE * mk * mk * U * scale, (mk, case, trial, res, C_SOLVE * mk * mk * U * scale)
        if case == "random" and mk >= 2:      # only the lower triangle is read
            A2 = A.copy(); A2[0, 1] = 1e300
            assert _same_bits(pkg.acceleration_query(A2, b), th)


def test_acceleration_query_argument_checks(pkg):
    import ctypes as C
    L = pkg.lib()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    A = np.eye(2); b = np.ones(2); th = np.zeros(2)
    assert L.admm_hip_acceleration_query(2, p(A), p(b), p(th)) == 0 and np.allclose(th, 1.0, rtol=1e-11)
    for mk in (0, -1, 9):
        assert L.admm_hip_acceleration_query(mk, p(A), p(b), p(th)) == 1
    assert L.admm_hip_acceleration_query(2, None, p(b), p(th)) == 1
    assert L.admm_hip_acceleration_query(2, p(A), None, p(th)) == 1
    assert L.admm_hip_acceleration_query(2, p(A), p(b), None) == 1
    # not positive definite (and not rescued by 1e-12 of the trace): zeros, and no error code -- the device then does not extrapolate
    assert _same_bits(pkg.acceleration_query(np.array([[1.0, 2.0], [2.0, 1.0]]), b), np.zeros(2))
    with pytest.raises(pkg.AdmmHipError):
        pkg.acceleration_query(np.eye(9), np.ones(9))
    with pytest.raises(pkg.AdmmHipError):
        pkg.acceleration_query(np.eye(3), np.ones(2))


def test_set_acceleration_arguments_and_host_only_context(pkg):
    """the setting only checks its argument, before or after initialize, on a host-only context too -- which still refuses to step"""
    mg = pkg.meshgen
    X, tets = mg.bar(1, 1, 1, h=0.1)
    s = pkg.System(device_id=-1)
    s.set_timestep(DT)
    s.add_nodes(X.ravel(), np.ones(3 * X.shape[0]))
    s.add_forces(KIND["TET_LINEAR"], tets, [1e4])
    for m in (0, 3, 8):
        s.set_acceleration(m)
    for bad in (-1, 9, 100):
        with pytest.raises(pkg.AdmmHipError, match="error 1"):
            s.set_acceleration(bad)
    s.initialize()
    s.set_acceleration(3)
    with pytest.raises(pkg.AdmmHipError, match="error 2"):
        s.step(3)
    with pytest.raises(pkg.AdmmHipError, match="error 2"):
        s.acceleration_log()
    s.set_acceleration(0)


def test_cpp_mirror_compiles(pkg):
    import os
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_anderson", pkg))


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def mixed_scene():
    """a 2 x 2 x 4-cell TET_LINEAR bar along z, anchored at its k = 0 face, a few springs across it, and a floor some nodes are below:
    every prox is exact (no truncated minimiser).  -> X (started bent down through the floor), M3, forces, shapes"""
    pkg = _pkg()
    mg = pkg.meshgen
    nx, ny, nz, h = 2, 2, 4, 0.1
    X, tets = mg.bar(nx, ny, nz, h=h)
    M3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    n = X.shape[0]
    layer = (nx + 1) * (ny + 1)
    springs = np.array([[k * layer, (k + 2) * layer + layer - 1] for k in range(nz - 1)] + [[layer + 2, 4 * layer + 6]], np.int32)
    forces = [("TET_LINEAR", tets, [2e4]), ("SPRING", springs, [500.0]), ("ANCHOR", mg.bar_anchor_nodes(nx, ny), [-1.0, 1.0]),
              ("COLLISION", np.arange(n, dtype=np.int32), [32.0])]
    shapes = ([pkg.SHAPE["FLOOR"]], [[0.0, -0.02, 0.0, 0.0]])
    Xs = X.copy()
    t = X[:, 2] / X[:, 2].max()
    Xs[:, 1] -= 0.09 * t * t
    Xs[:, 0] += 0.02 * np.sin(3.0 * t)
    return X, Xs, M3, forces, shapes


def mixed_system():
    X, Xs, M3, forces, shapes = mixed_scene()
    s = build_system(X, M3, forces, shapes)
    s.initialize()
    s.m_x = Xs.ravel()
    return s, forces


def lattice_system(stiffness=1e4):
    X, Xb, M3, forces = lattice_scene(stiffness)
    s = build_system(X, M3, forces)
    s.initialize()
    s.m_x = Xb.ravel()
    return s, forces


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_off_is_off(pkg):
    runs = []
    for mode in ("never", "zero", "three_then_zero"):
        s, forces = mixed_system()
        if mode == "zero":
            s.set_acceleration(0)
        if mode == "three_then_zero":
            s.set_acceleration(3); s.set_acceleration(0)
        for _ in range(6):
            s.step(5)
        runs.append((full_state(s, forces), s.graph_state()))
    for st, gs in runs[1:]:
        for a, b in zip(runs[0][0], st):
            assert _same_bits(a, b)
        assert gs == runs[0][1], (gs, runs[0][1])
    assert runs[0][1]["iter_graph"] and runs[0][1]["graph_launches"] > 0      # the comparison covers captured graphs
    # a context that turns acceleration on for one frame and off again keeps its graphs
    s, forces = mixed_system()
    s.step(5); s.step(5)
    g0 = s.graph_state()
    s.set_acceleration(3); s.step(5); s.set_acceleration(0)
    assert s.graph_state() == g0
    s.step(5)
    g1 = s.graph_state()
    assert g1["iter_graph"] and g1["frame_graph_iters"] == g0["frame_graph_iters"] and g1["graph_launches"] == g0["graph_launches"] + 1


@gpu
@pytest.mark.parametrize("iters", [1, 2])
def test_no_history_no_change(pkg, iters):
    """iteration 1 has m_k = 0 and the last iteration never extrapolates: one and two iterations per frame are the plain solver's"""
    plain, forces = mixed_system()
    acc, _ = mixed_system()
    acc.set_acceleration(3)
    for f in range(3):
        plain.step(iters); acc.step(iters)
        for a, b in zip(full_state(plain, forces), full_state(acc, forces)):
            assert _same_bits(a, b), f
        log = acc.acceleration_log()
        assert len(log) == iters and all(r["accepted"] or k > 0 for k, r in enumerate(log))
        assert not any(r["extrapolated"] for r in log) and log[0]["m_used"] == 0
        check_log_invariants(log, 3)
    assert acc.graph_state()["graph_launches"] == 0      # the accelerated loop runs eagerly


@gpu
def test_three_iterations_extrapolate_once(pkg):
    plain, forces = mixed_system()
    acc, _ = mixed_system()
    acc.set_acceleration(3)
    plain.step(3); acc.step(3)
    log = acc.acceleration_log()
    assert [r["m_used"] for r in log[:2]] == [0, 1] and log[1]["accepted"] and log[1]["extrapolated"] and not log[0]["extrapolated"]
    assert not log[2]["extrapolated"]
    check_log_invariants(log, 3)
    assert not _same_bits(plain.m_x, acc.m_x)
    assert np.isfinite(acc.m_x).all() and np.abs(acc.m_x - plain.m_x).max() < 0.05


@gpu
@needs_ld
def test_the_rule_restated(pkg):
    """Every quantity of the rule recomputed in long double from what the device itself produced: g_k (acceleration_default after a
    step whose last iteration k was accepted) and s_out_k (the z, u a tolerance exit after iteration k leaves: it ends the frame on
    the extrapolated iterate)."""
    K, M = 8, 3
    X, Xs, M3, forces, shapes = mixed_scene()
    s, _ = mixed_system()
    s.step(4); s.step(4)      # a state with u, v and contacts
    cp = checkpoint(s, forces)
    check_rule_restated(s, X, M3, forces, cp, K, M)


_LATTICE = {}


def lattice_plain():
    """plain ADMM on the lattice, one frame of 300 iterations: rho_k = |G(s_k-1) - s_k-1|^2_W from the (z, u) that k and k - 1
    iterations leave (each run restarts from the same state), the tracked residuals, K_plain.  Computed once for the tests below."""
    if _LATTICE:
        return _LATTICE
    s, forces = lattice_system()
    cp = checkpoint(s, forces)
    w2 = flat_weights(s, forces)
    X, Xb, M3, _ = lattice_scene()
    z0 = _frame_start_z(forces, X, M3, cp["x"])
    prev = np.concatenate([p for b in range(len(forces)) for p in (z0[b], cp["local"][b]["u"].ravel())])
    rho = []
    for k in range(1, 301):
        restore(s, forces, cp)
        s.step(k)
        cur = flat_state(s, forces)
        d = cur - prev
        rho.append(float(np.sum(w2 * d * d)))
        prev = cur
        if rho[-1] <= 1e-8 * rho[0]:
            break
    rho = np.array(rho)
    hit = np.nonzero(rho <= 1e-8 * rho[0])[0]
    restore(s, forces, cp)
    s.enable_residuals(True)
    s.step(300)
    r, sd, n = s.residuals(capacity=300)
    _LATTICE.update(rho=rho, K_plain=int(hit[0]) + 1 if hit.size else None, r=r, s=sd)
    return _LATTICE


def lattice_accelerated(window, stiffness=1e4, iters=300):
    s, forces = lattice_system(stiffness)
    s.set_acceleration(window)
    s.enable_residuals(True)
    s.step(iters)
    return s, forces, s.acceleration_log(capacity=iters)


@gpu
def test_it_accelerates(pkg):
    ref = lattice_plain()
    K_plain = ref["K_plain"]
    print("plain ADMM: rho_1 %.6e, K_plain %s" % (ref["rho"][0], K_plain))
    assert K_plain is not None and K_plain >= 100, K_plain
    s, forces, log = lattice_accelerated(3)
    rho = np.array([r["rho"] for r in log])
    assert _same_bits(rho[0], ref["rho"][0]) or abs(rho[0] - ref["rho"][0]) <= 1e-12 * ref["rho"][0]      # the same first iteration
    hit = np.nonzero(rho <= 1e-8 * ref["rho"][0])[0]
    K_acc = int(hit[0]) + 1 if hit.size else None
    print("window 3: reaches 1e-8 rho_1 at iteration %s; resets %d" % (K_acc, sum(not r["accepted"] for r in log)))
    assert K_acc is not None and K_acc <= K_plain / 2, (K_acc, K_plain)
    check_log_invariants(log, 3)
    assert np.isfinite(s.m_x).all()


@gpu
def test_the_safeguard(pkg):
    """the spring lattice (stiffness 1e4) at window 6 resets, as the float64 model of the rule did: on the device 54 times in 300
    iterations, first at iteration 126; after a reset z, u are the stored default bitwise and the history restarts"""
    s, forces, log = lattice_accelerated(6)
    resets = check_log_invariants(log, 6)
    print("lattice, window 6, 300 iterations: %d resets, first at iteration %s" % (resets, next((k + 1 for k, r in enumerate(log) if not r["accepted"]), None)))
    assert resets >= 1 and resets == sum(not r["accepted"] for r in log)
    first = next(k + 1 for k, r in enumerate(log) if not r["accepted"])
    assert first < len(log) and log[first]["accepted"] and log[first]["m_used"] == 0      # the next one is accepted, with no history
    # a frame that ends on the reset: z, u are s_def, bitwise
    s2, _ = lattice_system()
    s2.set_acceleration(6)
    s2.step(first)
    lg = s2.acceleration_log(capacity=first)
    assert len(lg) == first and not lg[-1]["accepted"]
    for a, b in zip(lg, log[:first]):
        assert _same_bits(a["rho"], b["rho"])
    assert _same_bits(flat_state(s2, forces), flat_state(s2, forces, default=True))
    # ... and one that exits on the tolerance right after it
    s3, _ = lattice_system()
    s3.set_acceleration(6)
    s3.set_tolerance(1e300, 1e300, first)
    s3.step(300)
    assert len(s3.acceleration_log()) == first
    assert _same_bits(flat_state(s3, forces), flat_state(s3, forces, default=True))
    assert _same_bits(flat_state(s3, forces), flat_state(s2, forces))


@gpu
def test_reproducible(pkg):
    runs = []
    for _ in range(2):
        s, forces = mixed_system()
        s.set_acceleration(6)
        logs = []
        for f in range(5):
            s.step(12)
            logs.append(s.acceleration_log())
        runs.append((full_state(s, forces), logs))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert _same_bits(a, b)
    for la, lb in zip(runs[0][1], runs[1][1]):
        assert len(la) == len(lb) == 12
        for a, b in zip(la, lb):
            assert (a["accepted"], a["m_used"], a["extrapolated"]) == (b["accepted"], b["m_used"], b["extrapolated"])
            for key in ("rho", "theta", "gram", "rhs"):
                assert _same_bits(a[key], b[key])
        check_log_invariants(la, 6)
    assert any(r["extrapolated"] for r in runs[0][1][0]) and np.isfinite(runs[0][0][0]).all()


@gpu
def test_checkpoint(pkg):
    """the history lives within a frame: x, v, u and the warm start resume an accelerated run bit for bit (a Neo-Hookean bar, so
    that there is a warm start)"""
    mg = pkg.meshgen
    dims = (2, 2, 6)

    def make():
        s = pkg.make_bar_system(*dims, device_id=0)
        s.initialize()
        s.set_acceleration(3)
        return s
    forces = [("TET_NH", None, None), ("ANCHOR", None, None)]
    a = make()
    for _ in range(3):
        a.step(8)
    cp = checkpoint(a, forces)
    for _ in range(2):
        a.step(8)
    b = make()
    restore(b, forces, cp)
    for _ in range(2):
        b.step(8)
    for p, q in zip(full_state(a, forces), full_state(b, forces)):
        assert _same_bits(p, q)
    assert any(r["extrapolated"] for r in b.acceleration_log())
    check_log_invariants(b.acceleration_log(), 3)


@gpu
def test_with_the_tolerance(pkg):
    ref = lattice_plain()
    K = ref["K_plain"]
    assert K is not None
    eps_r, eps_s = float(ref["r"][K - 1]), float(ref["s"][K - 1])
    plain, forces = lattice_system()
    plain.set_tolerance(eps_r, eps_s)
    plain.step(300)
    n_plain = plain.residuals(capacity=300)[2]
    acc, _ = lattice_system()
    acc.set_acceleration(3)
    acc.set_tolerance(eps_r, eps_s)
    acc.step(300)
    r, sd, n_acc = acc.residuals(capacity=300)
    print("tolerance (%.3e, %.3e): plain stops after %d iterations, window 3 after %d" % (eps_r, eps_s, n_plain, n_acc))
    assert n_acc < n_plain <= 300 and len(acc.acceleration_log()) == n_acc
    check_log_invariants(acc.acceleration_log(), 3)
    assert r[n_acc - 1] <= eps_r and sd[n_acc - 1] <= eps_s
    x1 = acc.m_x
    acc.step(300)      # the step after it runs normally: a new frame, a fresh history
    log = acc.acceleration_log()
    assert 1 <= len(log) <= 300 and log[0]["accepted"] and log[0]["m_used"] == 0
    check_log_invariants(log, 3)
    assert np.isfinite(acc.m_x).all() and not _same_bits(acc.m_x, x1)
    assert np.abs(acc.m_x - plain.m_x).max() < 1.0


@gpu
def test_refusals(pkg, monkeypatch):
    from test_sharding import _spring_net, _user_spring_system, _thread_allreduce_hooks, _run_sharded
    x, pairs = _spring_net(7)
    # a generic batch
    s = _user_spring_system(pkg, x, pairs, 400.0)
    s.initialize()
    s.step(4)
    x0, v0 = s.m_x, s.m_v
    s.set_acceleration(3)
    with pytest.raises(pkg.AdmmHipError, match="error 4"):
        s.step(4)
    assert _same_bits(s.m_x, x0) and _same_bits(s.m_v, v0)      # refused before anything ran
    s.set_acceleration(0)
    s.step(4)
    ref = _user_spring_system(pkg, x, pairs, 400.0)
    ref.initialize()
    ref.step(4); ref.step(4)
    assert _same_bits(s.m_x, ref.m_x)
    # world = 2 with the Python all-reduce hook
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "8")
    shards = [_user_spring_system(pkg, x, pairs, 400.0, rank=r, world=2, mode="subtree", generic=False) for r in range(2)]
    for sh, h in zip(shards, _thread_allreduce_hooks(2)):
        sh.set_allreduce(h)
    pkg.initialize_together(shards)
    for sh in shards:
        sh.set_acceleration(3)
        with pytest.raises(pkg.AdmmHipError, match="error 4"):
            sh.step(4)
        sh.set_acceleration(0)
    out = _run_sharded(shards, 2, 4, np.zeros(3 * shards[0].n_nodes))
    one = _user_spring_system(pkg, x, pairs, 400.0, generic=False)
    one.initialize()
    one.step(4); one.step(4)
    for r in range(2):
        assert np.isfinite(out[r][1][-1]).all() and np.abs(out[r][1][-1] - one.m_x).max() < 1e-9


@gpu
def test_cpp_mirror(pkg, tmp_path):
    from test_cpp_host import compile_cpp
    mg = pkg.meshgen
    dims = (2, 2, 6)
    X, tets = mg.bar(*dims)
    m3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    anchors = mg.bar_anchor_nodes(dims[0], dims[1]).astype(np.int32)
    frames, iters = 3, 7
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([X.shape[0], tets.shape[0], anchors.size, 0], dtype=np.int32).tofile(f)
        X.ravel().tofile(f); m3.tofile(f); tets.astype(np.int32).tofile(f); anchors.tofile(f)
    r = subprocess.run([compile_cpp("scene_anderson", pkg), str(inp), str(outp), str(frames), "-it", str(iters), "-aa", "3", "-v", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    xs = np.fromfile(outp).reshape(frames, -1)
    s = pkg.make_bar_system(*dims, device_id=0)
    s.initialize()
    s.set_acceleration(3)
    for fr in range(frames):
        s.step(iters)
        assert _same_bits(s.m_x, xs[fr]), fr
    log = s.acceleration_log()
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("iter ")]
    assert len(lines) == iters == len(log)
    for l, rec in zip(lines, log):
        assert (int(l[1]), int(l[2]), int(l[3])) == (int(rec["accepted"]), rec["m_used"], int(rec["extrapolated"])) and float.fromhex(l[4]) == rec["rho"]
    assert any(rec["extrapolated"] for rec in log)
    check_log_invariants(log, 3)
    plain = pkg.make_bar_system(*dims, device_id=0)
    plain.initialize()
    for fr in range(frames):
        plain.step(iters)
    assert not _same_bits(plain.m_x, xs[-1])      # -aa did something
