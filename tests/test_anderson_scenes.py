"""Anderson acceleration on every accelerable kind, on states of many blocks and at the windows 1, 6 and 8 (csrc/kernels_anderson.hpp,
csrc/abi_anderson.inc): the rule restated in long double (anderson_cases.check_rule_restated, the checker of tests/test_anderson.py) and
the right-hand side that the reslot kernels and the gather leave after the mix against checkers.RhsReference (anderson_cases.RhsAfterMix;
the operation count and the two conditions that keep that check from passing vacuously are in that module's docstring).

What tests/test_anderson.py's two scenes (every segment one or two blocks, TET_LINEAR / SPRING / ANCHOR / COLLISION only) leave out:
  all_kinds        element_cases.mixed_forces: eleven batches (more than MULTI_MAX: the local step goes batch by batch), all eleven kinds --
                   anderson_reslot_kernel at every (nodes, cols, idx_stride) and the frame-start z = D x of residual_dx_kernel for each;
                   again with per-corner tet slots (ADMM_HIP_PRERED=0: tets through anderson_reslot_kernel with nn = 4, cols = 3) and with
                   16-tet blocks (ADMM_HIP_TPB=16: anderson_reslot_tet_kernel with nact = tpb)
  long_segments    a 10 x 10 x 27-cell bar: two tet segments of 143 blocks each with a ragged last block, an odd-length collision segment
                   of ten blocks (its single trailing element at a non-zero block offset), more than 256 blocks in all (the strided first
                   stage of anderson_decide_kernel takes a second trip), the sparse solve; one stiffness per tet, so that
                   w2[i % n_local] matters in every row and block
  lattice 6x6x20   a spring segment of more than ten blocks: a reset (action 2 of anderson_mix_kernel) across blocks, and the windows
                   1 (the two-slot ring, which wraps at every accepted iteration) and 8 (= AA_MAX_M: the full extent of gr[], rh[], the
                   17 partial rows and AAState::gram)
Every case prints its block count, longest segment, extrapolated and reset iterations and the worst error / bound ratios.
"""
import numpy as np
import pytest

import element_cases
from anderson_cases import (AA_BLOCK, AA_PER_BLOCK, RhsAfterMix, _pkg, _same_bits, build_system, check_log_invariants, check_rule_restated,
                            checkpoint, flat_state, full_state, lattice_scene, needs_ld, restore, segments)
from checkers import KIND

pytestmark = [pytest.mark.gpu, needs_ld]

# the material table of tests/test_energy.py and tests/test_element_forces.py
PARAMS = dict(TET_NH=[1e5, 2e5, 5], TET_STVK=[1e5, 2e5, 5], TET_LINEAR=[4000.0], TET_VOLUME=[4000.0, 0.9, 1.1], TRI_FUNG=[50.0, 0.0, 0.0],
              TRI_STRAIN=[100.0, 0.95, 1.05, 1.0], TRI_AREA=[100.0, 3.0, 0.9, 1.1], SPRING=[300.0], BEND=[20.0])
ALL_KINDS_FLOOR = 0.02      # the bar's lowest layer of nodes (y about 0) lies below it, everything else above
# deform's amplitude.  Its default 0.04 scales the cloth's absolute coordinates (0.5 away from the origin, cells of 0.05) into strains of
# 40 %: in the frame's second iteration one TRI_FUNG triangle is nearly singular (singular values 1.36, 0.016) and the Fung projection
# returns NaN -- on the CPU oracle too.  At 0.02 and below the oracle stays finite over 2 x 4 + 40 iterations.
ALL_KINDS_AMP = 0.01


def report(name, s, forces, out, k_dof, log=None):
    """log: a longer frame's, where the case ran one beside the checker's"""
    seg = segments(s, forces)
    log = out["log"] if log is None else log
    print("%s: %d blocks, T %d doubles, longest segment %d doubles (%d blocks); %d extrapolated and %d reset iterations of %d; the rule restated over %d "
          "iterations, worst s_out error / bound %.3f; right-hand side checked %d times, worst error / bound %.3f, k_dof %s" %
          (name, seg["blocks"], seg["T"], seg["longest"], -(-seg["longest"] // AA_PER_BLOCK), sum(r["extrapolated"] for r in log),
           sum(not r["accepted"] for r in log), len(log), len(out["log"]), out["worst_sout"], out["rhs_checked"], out["worst_rhs"], k_dof))


def k_dof_range(rhs):
    return "7 + (T - 1) + (degree - 1), T = %d: %d .. %d" % (rhs.ref.T, rhs.ref.k_dof.min(), rhs.ref.k_dof.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# all_kinds
# ---------------------------------------------------------------------------------------------------------------------------------
def all_kinds_system():
    """element_cases.mixed_forces with a floor that the bar's lowest nodes are below, started from deform(X, ALL_KINDS_AMP) (no fold)"""
    pkg = _pkg()
    X, M3, forces = element_cases.mixed_forces(PARAMS)
    assert [k for k, _, _ in forces] == ["TET_NH", "TET_STVK", "TET_LINEAR", "TET_VOLUME", "TRI_STRAIN", "TRI_AREA", "TRI_FUNG", "BEND", "SPRING", "ANCHOR", "COLLISION"]
    assert set(k for k, _, _ in forces) == set(KIND)      # every kind there is
    s = element_cases.build_system(X, M3, forces, shapes=False)
    s.set_collision_shapes([pkg.SHAPE["FLOOR"]], [[0.0, ALL_KINDS_FLOOR, 0.0, 0.0]])
    s.initialize()
    x0 = element_cases.deform(X, amp=ALL_KINDS_AMP)
    below = int((x0[:, 1] < ALL_KINDS_FLOOR).sum())
    assert 0 < below < X.shape[0]
    s.m_x = x0.ravel()
    return s, X, M3, forces


def all_kinds_case(name):
    s, X, M3, forces = all_kinds_system()
    s.step(4); s.step(4)      # a state with u, v, warm starts and contacts
    cp = checkpoint(s, forces)
    rhs = RhsAfterMix(s, X, M3, forces)
    out = check_rule_restated(s, X, M3, forces, cp, 8, 3, rhs_ref=rhs)
    report(name, s, forces, out, k_dof_range(rhs))


def test_all_kinds(pkg):
    """eleven batches, every kind: the rule and the right-hand side after the mix, K = 8, M = 3"""
    all_kinds_case("all_kinds")


@pytest.mark.parametrize("iters", [1, 2])
def test_all_kinds_no_history_no_change(pkg, iters):
    """iteration 1 has m_k = 0 and the last iteration never extrapolates: one and two iterations per frame are the plain solver's, for
    every kind (x, v, every batch's u and z, bit for bit)"""
    plain, X, M3, forces = all_kinds_system()
    acc = all_kinds_system()[0]
    acc.set_acceleration(3)
    for f in range(3):
        plain.step(iters); acc.step(iters)
        for a, b in zip(full_state(plain, forces), full_state(acc, forces)):
            assert _same_bits(a, b), f
        log = acc.acceleration_log()
        assert len(log) == iters and not any(r["extrapolated"] for r in log) and log[0]["m_used"] == 0
        check_log_invariants(log, 3)


@pytest.mark.parametrize("knob,value", [("ADMM_HIP_PRERED", "0"), ("ADMM_HIP_TPB", "16")])
def test_all_kinds_other_layouts(pkg, monkeypatch, knob, value):
    """per-corner tet slots / 16-tet blocks for the NH and StVK batches: both reference checks again (the layouts cut the sums elsewhere:
    their bits differ from the default's, and nothing here compares them)"""
    monkeypatch.setenv(knob, value)      # (read when the context is created)
    all_kinds_case("all_kinds %s=%s" % (knob, value))


# ---------------------------------------------------------------------------------------------------------------------------------
# long_segments
# ---------------------------------------------------------------------------------------------------------------------------------
def long_bar_scene():
    """a 10 x 10 x 27-cell TET_LINEAR bar along z (16 200 tets, 3 388 nodes), one stiffness per tet, anchored at its k = 0 face; a
    collision batch over the 3 267 other nodes and a floor that the bent start goes through"""
    pkg = _pkg()
    mg = pkg.meshgen
    nx, ny, nz, h = 10, 10, 27, 0.05
    X, tets = mg.bar(nx, ny, nz, h=h)
    M3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    anchors = mg.bar_anchor_nodes(nx, ny)
    free = np.setdiff1d(np.arange(X.shape[0], dtype=np.int32), anchors).astype(np.int32)
    stiffness = 2e4 * (1.0 + 0.5 * np.sin(0.37 * np.arange(tets.shape[0])))
    forces = [("TET_LINEAR", tets, stiffness[:, None]), ("ANCHOR", anchors, [-1.0, 1.0]), ("COLLISION", free, [32.0])]
    shapes = ([pkg.SHAPE["FLOOR"]], [[0.0, -0.04, 0.0, 0.0]])
    Xs = X.copy()
    t = X[:, 2] / X[:, 2].max()
    Xs[:, 1] -= 0.25 * t * t
    Xs[:, 0] += 0.03 * np.sin(3.0 * t)
    assert 0 < (Xs[free, 1] < -0.04).sum() < free.size
    return X, Xs, M3, forces, shapes


def test_long_segments(pkg):
    """K = 6, M = 3 on a state of more than 256 blocks, above the dense limit"""
    X, Xs, M3, forces, shapes = long_bar_scene()
    assert np.asarray(forces[0][1]).shape == (16200, 4) and X.shape[0] == 3388
    s = build_system(X, M3, forces, shapes)
    s.initialize()
    assert not s.info()["dense_solve"]
    s.m_x = Xs.ravel()
    seg = segments(s, forces)
    assert seg["blocks"] >= 286 and seg["blocks"] > AA_BLOCK and seg["longest"] == 145800
    assert ((seg["cnt"] > AA_PER_BLOCK) & (seg["cnt"] % 2 == 1)).any()      # an odd-length segment of several blocks
    assert (seg["cnt"][seg["cnt"] > AA_PER_BLOCK] % AA_PER_BLOCK != 0).all()      # ragged last blocks
    w = s.read_rest(0)["weight"]
    assert np.unique(w).size > w.size // 2      # the weights differ from tet to tet
    s.step(4); s.step(4)
    cp = checkpoint(s, forces)
    rhs = RhsAfterMix(s, X, M3, forces)
    out = check_rule_restated(s, X, M3, forces, cp, 6, 3, rhs_ref=rhs)
    report("long_segments", s, forces, out, k_dof_range(rhs))


# ---------------------------------------------------------------------------------------------------------------------------------
# the lattice scaled to 6 x 6 x 20 nodes: a reset across blocks, the windows 1 and 8
# ---------------------------------------------------------------------------------------------------------------------------------
LATTICE_DIMS = (6, 6, 20)


def big_lattice(stiffness=1e4):
    X, Xb, M3, forces = lattice_scene(stiffness, LATTICE_DIMS)
    s = build_system(X, M3, forces)
    s.initialize()
    s.m_x = Xb.ravel()
    seg = segments(s, forces)
    assert seg["longest"] > 10 * AA_PER_BLOCK      # the spring segment has more than ten blocks
    return s, X, M3, forces


def test_reset_on_long_segments(pkg):
    """lattice_scene at 6 x 6 x 20 nodes, stiffness 1e4, window 6 (the values of test_the_safeguard): one frame of 300 iterations resets at
    least once; the rule over its first 12 iterations"""
    s, X, M3, forces = big_lattice(1e4)
    cp = checkpoint(s, forces)
    s.set_acceleration(6)
    s.step(300)
    log = s.acceleration_log(capacity=300)
    assert len(log) == 300
    resets = check_log_invariants(log, 6)
    first = next((k + 1 for k, r in enumerate(log) if not r["accepted"]), None)
    print("lattice 6 x 6 x 20, window 6, 300 iterations: %d resets, first at iteration %s" % (resets, first))
    assert resets >= 1 and resets == sum(not r["accepted"] for r in log)
    # the frame that ends on the first reset: z, u are the stored default, bitwise, in every block, and the right-hand side is the
    # reference's of that state (the shares written again from s_def, not left as the rejected local step wrote them)
    restore(s, forces, cp)
    s.step(first)
    lg = s.acceleration_log(capacity=first)
    assert len(lg) == first and not lg[-1]["accepted"]
    s_def = flat_state(s, forces, default=True)
    assert _same_bits(flat_state(s, forces), s_def)
    rhs = RhsAfterMix(s, X, M3, forces)
    rhs.check(first, rhs.xbar(cp), s.debug_rhs(), s_def)
    reset_ratio = rhs.worst
    out = check_rule_restated(s, X, M3, forces, cp, 12, 6, rhs_ref=rhs)
    for a, b in zip(out["log"], log[:12]):      # the long frame began with the very iterations the rule was restated on
        assert _same_bits(a["rho"], b["rho"]) and _same_bits(a["theta"], b["theta"])
    report("reset_on_long_segments", s, forces, out, k_dof_range(rhs), log=log)
    print("reset_on_long_segments: the right-hand side of the frame that ends on the reset at iteration %d: error / bound %.3f" % (first, reset_ratio))


@pytest.mark.parametrize("M,K", [(1, 6), (8, 12)])
def test_windows_one_and_eight(pkg, M, K):
    """the two-slot ring and the full window on the 6 x 6 x 20 lattice (stiffness 1e4): m_used reaches 8 at iteration 9 there"""
    s, X, M3, forces = big_lattice(1e4)
    cp = checkpoint(s, forces)
    rhs = RhsAfterMix(s, X, M3, forces)
    out = check_rule_restated(s, X, M3, forces, cp, K, M, rhs_ref=rhs)
    assert max(r["m_used"] for r in out["log"]) == M
    report("window %d" % M, s, forces, out, k_dof_range(rhs))
