"""What tests/test_anderson.py and tests/test_anderson_scenes.py share: building a scene, checkpoints, the flat state and its weights,
the log's invariants, and the rule of Anderson acceleration restated in long double (check_rule_restated).  A plain module, imported
like checkers and element_cases.

The state s = (z, u) is handled here as one flat vector: batch after batch, the batch's z [n][rows] then its u, with the weights w^2
of the batch's elements repeated over the rows.  Sums do not depend on that order; elementwise checks do not either.  The device keeps
every part as [rows][n] in segments of AA_PER_BLOCK doubles per block (csrc/kernels_anderson.hpp); segments() restates that layout's
sizes from read_rest and the kind tables.

The right-hand side after the mix (RhsAfterMix).  A frame that leaves on the tolerance after iteration k has z, u = s_out_k, the
elements' shares written again from s_out_k by anderson_reslot_kernel / anderson_reslot_tet_kernel, the right-hand side gathered from
them and the solve done (abi_step.inc leaves the loop only after launch_solve, which reads the vector and leaves it).  debug_rhs() is
then b = M x_bar + dt^2 D^T W^2 (z - u) of the MIXED state, and checkers.RhsReference recomputes it in np.longdouble from read_local's
z, u with the oracle's D, W and masses; x_bar is checkers.explicit_reference's, from the checkpoint's x and v.
The bound is RhsReference.bound, unchanged: k(node) = 7 + (T - 1) + (degree - 1) roundings.  Its count was made for the projection
kernels; the reslot kernels cost the same, operation by operation:
  anderson_reslot_kernel      q = fl(z - u)  1;  s = w2h2 = fl(fl(dt dt) fl(w w))  3;  g q and s (sum)  2;  the sum over `cols` <= 3 terms
                              from 0.0: cols - 1 <= T - 1 additions;  one slot per corner, so the gather adds degree - 1 times
  anderson_reslot_tet_kernel  the same 1 + 3 + 2 and (g0 q0 + g1 q1) + g2 q2: 2 = T - 1 additions;  the block's run in LDS plus the node's
                              slots in the gather: never more than degree - 1 additions
and rhs_gather_kernel adds fl(m x_bar) last (1).  Nothing is added to k_dof.
x_bar itself: the device's carries the four roundings of v + dt g and x + dt v against the long-double one.  checkers.explicit_bound
bounds that distance per dof; the check asserts -- from the reference alone -- that m times it stays below 5 % of the right-hand side's
bound in every dof (on the CPU oracle's states of these scenes it is 0.5 % at the most): the comparison stays the one against
RhsReference.bound, and x_bar's own rounding can move it by a twentieth of that bound at the most.
Two conditions keep the check from passing vacuously, both from the reference alone: the corner sensitivity of
tests/test_rhs_reference.py (every corner of every batch's last element and 99 % of all corners are worth 1000 bounds or more), and
the distance between the reference b of g_k and of s_out_k (more than 10 bounds in at least 10 % of the dofs: shares left as the
projection kernels wrote them would fail).
"""
import numpy as np
import pytest

from checkers import KIND, KIND_NODES, KIND_ROWS, Oracle, RhsReference, explicit_bound

LD = np.longdouble
U = 2.0 ** -53
needs_ld = pytest.mark.skipif(np.finfo(LD).eps > 2.0 ** -63, reason="np.longdouble has no extended precision on this host")
DT = 0.04
GRAVITY = (0.0, -9.8, 0.0)
AA_PER_BLOCK = 1024      # doubles per block of the elementwise kernels (kernels_anderson.hpp)
AA_BLOCK = 256           # threads of anderson_decide_kernel: its strided first stage takes a second trip beyond 256 blocks


def _pkg():
    from __graft_entry__ import load_package
    return load_package()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def build_system(X, M3, forces, shapes=None, device_id=0):
    s = _pkg().System(device_id=device_id)
    s.set_timestep(DT)
    s.add_nodes(np.asarray(X).ravel(), M3)
    for kind, idx, par in forces:
        s.add_forces(KIND[kind], idx, par)
    if shapes is not None:
        s.set_collision_shapes(*shapes)
    s.add_gravity(list(GRAVITY))
    return s


def lattice_scene(stiffness=1e4, dims=(3, 3, 10)):
    """the spring lattice: nx x ny x nl nodes, axis and diagonal springs, the bottom layer anchored, started bent"""
    nx, ny, nl = dims
    h = 0.1
    idx = lambda i, j, l: (l * ny + j) * nx + i      # noqa: E731
    X = np.array([[i * h, l * h, j * h] for l in range(nl) for j in range(ny) for i in range(nx)], dtype=np.float64)
    springs = []
    for l in range(nl):
        for j in range(ny):
            for i in range(nx):
                for di, dj, dl in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, -1, 0), (1, 0, -1), (0, 1, -1)):
                    i2, j2, l2 = i + di, j + dj, l + dl
                    if 0 <= i2 < nx and 0 <= j2 < ny and 0 <= l2 < nl:
                        springs.append((idx(i, j, l), idx(i2, j2, l2)))
    anchors = np.array([idx(i, j, 0) for j in range(ny) for i in range(nx)], np.int32)
    Xb = X.copy()
    Xb[:, 0] += 0.3 * (X[:, 1] / X[:, 1].max()) ** 2
    forces = [("SPRING", np.array(springs, np.int32), [stiffness]), ("ANCHOR", anchors, [-1.0, 1.0])]
    return X, Xb, np.full(3 * X.shape[0], 0.1), forces


# ---------------------------------------------------------------------------------------------------------------------------------
# the solver's state
# ---------------------------------------------------------------------------------------------------------------------------------
def checkpoint(s, forces):
    """x, v, every batch's u and warm start: what DESIGN lists (the scenes here have no sides)"""
    return dict(x=s.m_x, v=s.m_v, local=[s.read_local(b) for b in range(len(forces))])


def restore(s, forces, cp):
    s.m_x = cp["x"]; s.m_v = cp["v"]
    for b, (kind, _, _) in enumerate(forces):
        loc = cp["local"][b]
        s.write_local(b, u=loc["u"], state=loc["state"] if loc["state"].shape[1] == 4 else None)


def full_state(s, forces):
    out = [s.m_x, s.m_v]
    for b in range(len(forces)):
        loc = s.read_local(b)
        out += [loc["u"], loc["z"]]
    return out


def flat_state(s, forces, default=False):
    """(z, u) of all batches as one vector"""
    parts = []
    for b in range(len(forces)):
        loc = s.acceleration_default(b) if default else s.read_local(b)
        parts += [loc["z"].ravel(), loc["u"].ravel()]
    return np.concatenate(parts)


def flat_weights(s, forces):
    """w^2 of every entry of the flat state: read_rest's weight is one per ELEMENT (per-element parameter rows give per-element
    weights), repeated over the element's rows, once for z and once for u"""
    parts = []
    for b, (kind, idx, _) in enumerate(forces):
        w = s.read_rest(b)["weight"]
        assert w.shape == (np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]]).shape[0],)
        w2 = np.repeat(w * w, KIND_ROWS[KIND[kind]])
        parts += [w2, w2]
    return np.concatenate(parts)


def segments(s, forces):
    """the device's segment table restated from read_rest and the kind tables (ensure_anderson_buffers): per batch a z and a u segment
    of rows * n doubles, ceil(cnt / AA_PER_BLOCK) blocks each, at even offsets.  -> dict(cnt [2 per batch], blocks, T, longest)"""
    cnt = []
    for b, (kind, _, _) in enumerate(forces):
        c = KIND_ROWS[KIND[kind]] * s.read_rest(b)["weight"].size
        cnt += [c, c]
    cnt = np.array(cnt, dtype=np.int64)
    return dict(cnt=cnt, blocks=int((-(-cnt // AA_PER_BLOCK)).sum()), T=int((cnt + (cnt & 1)).sum()), longest=int(cnt.max()))


def check_log_invariants(log, window):
    """what holds in every log: rho of accepted iterations falls strictly between resets, the decisions follow from the logged rhos
    exactly, m_used restarts at 0 after a reset and grows by one per accepted iteration up to the window.  -> number of resets"""
    resets, armed, rho_acc, entries = 0, False, None, 0
    for k, r in enumerate(log):
        accept = (not armed) or r["rho"] < rho_acc
        assert r["accepted"] == accept, (k, r["rho"], rho_acc)
        if accept:
            if armed:
                assert r["rho"] < rho_acc
            entries += 1
            assert r["m_used"] == min(entries - 1, window), (k, r["m_used"], entries)
            assert r["extrapolated"] == (r["m_used"] >= 1 and k + 1 < len(log) and not r["solve_failed"]) or k + 1 == len(log), k
            armed, rho_acc = True, r["rho"]
        else:
            resets += 1
            assert r["m_used"] == 0 and not r["extrapolated"]
            armed, entries = False, 0
    return resets


# ---------------------------------------------------------------------------------------------------------------------------------
# the CPU oracle of a scene: selector rows, weights, masses
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_oracle(forces, X, M3):
    """the CPU oracle of the scene (params broadcast or one row per element, every kind): only its D, W, row layout and masses are
    used here, so the collision shapes are not needed"""
    o = Oracle(); o.settings(DT, 1)
    o.add_nodes(np.asarray(X).ravel(), M3)
    for kind, idx, par in forces:
        o.add_forces(KIND[kind], idx, par)
    o.add_gravity(list(GRAVITY))
    assert o.initialize()
    return o


def batch_first(forces):
    """the oracle's force index of every batch's element 0 (and the total)"""
    return np.concatenate([[0], np.cumsum([np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]]).shape[0] for kind, idx, _ in forces])]).astype(np.int64)


def _frame_start_z(forces, X, M3, x, oracle=None):
    """D x of the frame-start x in the flat layout's z parts, in long double rounded to double (the CPU oracle's selector rows)"""
    o = scene_oracle(forces, X, M3) if oracle is None else oracle
    rr, cc, vv = o.D_triplets()
    Dx = np.zeros(o.rows, dtype=LD)
    np.add.at(Dx, rr, vv.astype(LD) * np.asarray(x, dtype=np.float64).astype(LD)[cc])
    Dx = np.asarray(Dx, dtype=np.float64)
    gi = np.asarray(o.global_idx(), dtype=np.int64)
    first = batch_first(forces)
    out = []
    for b, (kind, _, _) in enumerate(forces):
        rows = KIND_ROWS[KIND[kind]]
        out.append(Dx[gi[first[b]:first[b + 1]][:, None] + np.arange(rows)[None, :]].ravel())
    return out


class RhsAfterMix:
    """the right-hand side a frame leaves behind against checkers.RhsReference (the module's docstring).  Built once per scene."""

    def __init__(self, s, X, M3, forces):
        self.forces, self.oracle = forces, scene_oracle(forces, X, M3)
        self.ref = RhsReference(self.oracle, DT)
        self.first = batch_first(forces)
        # the device's weights and row layout are bitwise the oracle's (everything else in the reference is the oracle's alone)
        for b, (kind, _, _) in enumerate(forces):
            rest = s.read_rest(b)
            f0, f1 = self.first[b], self.first[b + 1]
            assert np.array_equal(rest["weight"], self.ref.weights[f0:f1]) and np.array_equal(rest["global_idx"], self.ref.gidx[f0:f1]), kind
        self.worst, self.checked, self.far = 0.0, 0, 1.0

    def xbar(self, cp):
        """x_bar of the frame that starts from the checkpoint, in long double (explicit_reference's, through explicit_bound); the bound on
        the device's own rounded x_bar times the masses is kept for check()"""
        (xbar, _, _), (bx, _, _) = explicit_bound(cp["x"], cp["v"], DT, [("const", GRAVITY, None)])
        self.m_dxbar = self.ref.m3.astype(LD) * bx
        return xbar

    def rows(self, flat):
        """a flat state -> (u, z) in the oracle's row order"""
        u = np.full(self.ref.rows, np.nan); z = np.full(self.ref.rows, np.nan)
        p = 0
        for b, (kind, _, _) in enumerate(self.forces):
            n, rows = int(self.first[b + 1] - self.first[b]), KIND_ROWS[KIND[kind]]
            at = self.ref.rows_of(self.first[b], np.arange(n), KIND[kind])
            z[at] = flat[p:p + n * rows].reshape(n, rows); p += n * rows
            u[at] = flat[p:p + n * rows].reshape(n, rows); p += n * rows
        assert p == flat.size and np.isfinite(u).all() and np.isfinite(z).all()
        return u, z

    def check(self, k, xbar, y, s_out, g=None):
        """y: debug_rhs() of the frame that left after iteration k with z, u = s_out; g: the local step's own output of that iteration
        (None after a reset: the rejected output is not kept anywhere, so the distance condition has nothing to measure)"""
        ref = self.ref
        assert np.isfinite(y).all()
        u, z = self.rows(s_out)
        b_ref, bound = ref.b(xbar, u, z), ref.bound(xbar, u, z)
        assert (bound > 0).all()
        assert float((self.m_dxbar / bound).max()) <= 0.05      # the device's rounded x_bar against the long-double one (the module's docstring)
        # the two conditions, from the reference alone
        sens = ref.corner_sensitivity(xbar, u, z)
        for b, (kind, _, _) in enumerate(self.forces):
            tail = ref.corner_force == self.first[b + 1] - 1
            assert tail.sum() == KIND_NODES[KIND[kind]]
            assert sens[tail].min() >= 1000, (k, kind, sens[tail])
        frac = float((sens >= 1000).mean())
        assert frac >= 0.99, (k, frac)
        far = float("nan")
        if g is not None:
            ug, zg = self.rows(g)
            far = float((np.abs(ref.b(xbar, ug, zg) - b_ref) > 10 * bound).mean())
            assert far >= 0.10, (k, far)
        # the device
        ratio = np.abs(y.astype(LD) - b_ref) / bound
        worst = int(np.argmax(ratio))
        print("iteration %d: right-hand side after the mix: max |b_dev - b_ref| / bound %.3f at dof %d (node degree %d, k %d); %.1f %% of the dofs "
              "more than 10 bounds from b(g_k); %.2f %% of the corners worth 1000 bounds" %
              (k, float(ratio[worst]), worst, ref.degree[worst // 3], ref.k_dof[worst], 100 * far, 100 * frac))
        assert ratio[worst] <= 1.0, (k, float(ratio[worst]), worst)
        self.worst = max(self.worst, float(ratio[worst])); self.far = min(self.far, far) if g is not None else self.far; self.checked += 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule restated
# ---------------------------------------------------------------------------------------------------------------------------------
def check_rule_restated(s, X, M3, forces, cp, K, M, rhs_ref=None, fill=None):
    """Every quantity of the rule recomputed in long double from what the device itself produced: g_k (acceleration_default after a
    step whose last iteration k was accepted) and s_out_k (the z, u a tolerance exit after iteration k leaves: it ends the frame on
    the extrapolated iterate).  s: an initialized system; cp: the checkpoint every run starts from (the window is set here).
    rhs_ref: a RhsAfterMix -- the right-hand side of every frame that left on an extrapolated iterate is checked too.
    fill: the largest m_used the log must show (the window unless given).
    -> dict(log, resets, n_ex, worst_sout: the largest |s_out - ref| / bound, worst_rhs, rhs_checked)"""
    pkg = _pkg()
    fill = M if fill is None else fill
    if rhs_ref is not None:
        rhs_ref.worst, rhs_ref.checked, rhs_ref.far = 0.0, 0, 1.0
    s.set_acceleration(M)
    w2 = flat_weights(s, forces)
    logs, live, deflt = {}, {}, {}
    for k in range(1, K + 1):
        restore(s, forces, cp)
        s.step(k)
        logs[k] = s.acceleration_log(); live[k] = flat_state(s, forces); deflt[k] = flat_state(s, forces, default=True)
        assert len(logs[k]) == k
    # every run is a bitwise prefix of the next (the last iteration solves too; only its `extrapolated` differs)
    for k in range(1, K):
        for a, b in zip(logs[k], logs[k + 1][:k]):
            for key in ("rho", "theta", "gram", "rhs"):
                assert _same_bits(a[key], b[key]), (k, key)
            assert (a["accepted"], a["m_used"], a["solve_failed"]) == (b["accepted"], b["m_used"], b["solve_failed"])
        assert not logs[k][-1]["extrapolated"]
    log = logs[K]
    # s_out_k of the iterations that are not the last: a tolerance that everything meets, tested after iteration k only
    sout, rhs = {K: live[K]}, {}
    for k in range(1, K):
        restore(s, forces, cp)
        s.set_tolerance(1e300, 1e300, k)
        s.step(K)
        lg = s.acceleration_log()
        assert len(lg) == k
        for a, b in zip(lg, log[:k]):      # tracking changes nothing the rule sees
            assert _same_bits(a["rho"], b["rho"]) and _same_bits(a["theta"], b["theta"]) and a["extrapolated"] == b["extrapolated"]
        sout[k] = flat_state(s, forces)
        if rhs_ref is not None and log[k - 1]["extrapolated"]:
            rhs[k] = s.debug_rhs()
        s.set_tolerance(0.0, 0.0, 1)
    resets = check_log_invariants(log, M)
    xbar = rhs_ref.xbar(cp) if rhs_ref is not None else None
    # s_in of iteration 1: z = D x, u as restored
    z0 = _frame_start_z(forces, X, M3, cp["x"], oracle=rhs_ref.oracle if rhs_ref is not None else None)
    s_in = np.concatenate([p for b in range(len(forces)) for p in (z0[b], cp["local"][b]["u"].ravel())])
    assert s_in.size == w2.size == live[K].size
    hist = []      # (g, f) of the accepted iterations since the last reset, at most M + 1
    n_ex, worst_sout = 0, 0.0
    for k in range(1, K + 1):
        r = log[k - 1]
        if not r["accepted"]:
            assert _same_bits(sout[k], deflt[k]) and _same_bits(live[k], deflt[k])      # s_out = s_def, bitwise
            hist = []
            s_in = sout[k]
            continue
        g = deflt[k]      # iteration k was the last of run k and accepted: s_def = g_k
        assert _same_bits(live[k], g)      # ... and the last iteration left it in z, u
        f = g - s_in      # (the device forms f in double too: one rounding, the same one)
        terms = w2.astype(LD) * (f.astype(LD) * f.astype(LD))
        rho = float(np.sum(terms)); bound = terms.size * U * float(np.sum(np.abs(terms)))
        print("iteration %d: rho %.17g logged %.17g |diff| %.3e bound %.3e" % (k, rho, r["rho"], abs(rho - r["rho"]), bound))
        assert abs(rho - r["rho"]) <= bound, (k, rho, r["rho"], bound)
        hist.append((g, f)); hist = hist[-(M + 1):]
        mk = len(hist) - 1
        assert r["m_used"] == mk
        if mk == 0:
            assert _same_bits(sout[k], g)
            s_in = sout[k]
            continue
        dF = [hist[j + 1][1] - hist[j][1] for j in range(mk)]      # double differences, as on the device
        dG = [hist[j + 1][0] - hist[j][0] for j in range(mk)]
        for a in range(mk):
            t = w2.astype(LD) * (dF[a].astype(LD) * f.astype(LD))
            ref, bnd = float(np.sum(t)), t.size * U * float(np.sum(np.abs(t)))
            assert abs(ref - r["rhs"][a]) <= bnd, (k, a, ref, r["rhs"][a], bnd)
            for b in range(mk):
                t = w2.astype(LD) * (dF[a].astype(LD) * dF[b].astype(LD))
                ref, bnd = float(np.sum(t)), t.size * U * float(np.sum(np.abs(t)))
                assert abs(ref - r["gram"][a, b]) <= bnd, (k, a, b, ref, r["gram"][a, b], bnd)
                assert _same_bits(r["gram"][a, b], r["gram"][b, a])
        assert not r["solve_failed"]
        assert _same_bits(r["theta"], pkg.acceleration_query(r["gram"], r["rhs"])), k      # the host twin, bitwise
        if k == K:
            assert not r["extrapolated"]
            continue
        assert r["extrapolated"]
        n_ex += 1
        th = r["theta"]
        ref = g.astype(LD) - sum(LD(th[j]) * dG[j].astype(LD) for j in range(mk))
        bnd = (mk + 2) * U * (np.abs(g) + sum(abs(th[j]) * np.abs(dG[j]) for j in range(mk)))
        err = np.abs(np.asarray(sout[k], dtype=LD) - ref).astype(np.float64)
        worst = float(np.max(err / np.maximum(bnd, 1e-300)))
        print("iteration %d: m_k %d theta %s  max |s_out - ref| / bound %.3f" % (k, mk, th, worst))
        assert (err <= bnd).all(), (k, float(err.max()))
        worst_sout = max(worst_sout, worst)
        if rhs_ref is not None:
            rhs_ref.check(k, xbar, rhs[k], sout[k], g)
        s_in = sout[k]
    assert n_ex >= 3 and max(r["m_used"] for r in log) == fill      # the window filled
    assert rhs_ref is None or rhs_ref.checked == n_ex
    return dict(log=log, resets=resets, n_ex=n_ex, worst_sout=worst_sout, worst_rhs=rhs_ref.worst if rhs_ref is not None else None,
                rhs_checked=rhs_ref.checked if rhs_ref is not None else 0)
