"""GPU: the DEVICE-only branches of csrc/local_math.hpp, one function per launch through admm_hip_debug_math
(System.debug_math), every bit.

The header is compiled twice and the two builds differ in four places: sqrt_core (v_rsq_f64 + a hand-written Newton sequence
without the compiler's rescaling and special cases, against libm's sqrt), rcp_in_1_2 (v_rcp_f64 + Newton steps without
v_div_scale / v_div_fixup, against 1.0 / b), the wave-uniform path of mt_cstep (__ballot picks mt_cstep_case<C>; the host only
emulates it) and every plain sqrt and division inside mt_cstep, svd3 and svd32 (hipcc's expansions against libm and the x86
divider).  tests/test_host_math.py pins the host build to the oracle; this file pins the device build to the host build:

  ops 2-4  the scalar helpers against an integer-exact reference on the hard sets (results next to a rounding midpoint,
           tests/math_cases.py) and against np.sqrt / 1.0 / b -- shown correct on the hard sets by test_host_math.py -- on 2M more
  ops 5-8  eig_hypot, svd3, oriented_svd, svd32 against the host build on 1M records each
  op 9     mt_cstep on waves composed lane by lane (the hook runs record i on lane i % 64 of wave i / 64)"""
import numpy as np
import pytest

import math_cases
from test_host_math import hm, mismatches, run_hm  # noqa: F401  (hm: fixture, the host build of local_math.hpp)

pytestmark = pytest.mark.gpu

WAVE = math_cases.WAVE


@pytest.fixture(scope="module")
def dev(pkg):
    s = pkg.make_bar_system(2, 2, 3)
    s.initialize()
    return s


def check(name, x, got, want):
    """every bit (any NaN for a NaN); on failure the count and the first five (argument, got, want) as hex floats"""
    bad = mismatches(got, want)
    if bad.size:
        x, got, want = (np.asarray(a).reshape(len(a), -1) for a in (x, got, want))
        lines = ["%s: %d of %d records differ" % (name, bad.size, len(x))]
        for i in bad[:5]:
            lines.append("  [%d] arg %s\n      got  %s\n      want %s" % (i, " ".join(float(v).hex() for v in x[i]), " ".join(float(v).hex() for v in got[i]),
                                                                       " ".join(float(v).hex() for v in want[i])))
        print("\n".join(lines))
    assert bad.size == 0, "%s: %d of %d records differ (first: %d)" % (name, bad.size, len(got), bad[0])


SCALAR = {
    "sqrt_in_1_4": (math_cases.sqrt_in_1_4_args, math_cases.sqrt_hard, math_cases.exact_sqrt, np.sqrt),
    "sqrt_ge_1": (math_cases.sqrt_ge_1_args, math_cases.sqrt_hard, math_cases.exact_sqrt, np.sqrt),
    "rcp_in_1_2": (math_cases.rcp_in_1_2_args, math_cases.rcp_hard, math_cases.exact_rcp, lambda b: 1.0 / b),
}


@pytest.mark.parametrize("name", list(SCALAR))
def test_scalar_helper_is_correctly_rounded_on_the_hard_set(pkg, dev, name):
    """results within 1.4e-12 ulp (square root) / 2^-27 and 2^-14 ulp (reciprocal) of a rounding midpoint: an algorithm whose error
    reaches 0.5 ulp + a little fails on about every second one of these.  Reference: integers."""
    hard = SCALAR[name][1]()
    want = np.array([SCALAR[name][2](v) for v in hard])
    got = dev.debug_math(pkg.DEBUG_MATH_OP[name], hard.reshape(-1, 1))
    check(name + " (hard set)", hard, got, want)


@pytest.mark.parametrize("name", list(SCALAR))
def test_scalar_helper_on_its_whole_range(pkg, dev, name):
    """2M arguments over the stated range -- uniform, the doubles around the range's ends and around 2 resp. sqrt 2, exact squares and
    their neighbours, the forms production evaluates -- against np.sqrt / 1.0 / b; NaN (any payload) gives NaN, sqrt_ge_1(+inf) is
    +inf.  Launches of 1, 63, 64 and 65 records: a lone lane, a wave short of one lane, a full one, one lane into the next."""
    x = SCALAR[name][0]()
    with np.errstate(invalid="ignore"):
        want = SCALAR[name][3](x)
    op = pkg.DEBUG_MATH_OP[name]
    for n in (1, 63, 64, 65, x.size):
        got = dev.debug_math(op, x[:n].reshape(-1, 1))
        check("%s (n = %d)" % (name, n), x[:n], got, want[:n])
        assert np.array_equal(np.isnan(got[:, 0]), np.isnan(x[:n]))
    if name == "sqrt_ge_1":
        assert np.isinf(x).sum() > 1000 and np.all(got[np.isinf(x), 0] == np.inf)


@pytest.mark.parametrize("name,cases,n_out", [("eig_hypot", math_cases.hypot_pairs, 1), ("svd3", math_cases.svd3_matrices, 21),
                                              ("oriented_svd", math_cases.svd3_matrices, 21), ("svd32", math_cases.svd32_matrices, 12)])
def test_device_equals_host_build(pkg, dev, hm, name, cases, n_out):
    """hipcc's sqrt and division expansions, and sqrt_core / rcp_in_1_2 in their callers, inside eig_hypot and the Jacobi SVDs: the
    device's output against the host build of the same header (which test_host_math.py ties to the oracle) on 1M records, NaN
    positions included."""
    x = cases()
    want = run_hm(hm, "hypot" if name == "eig_hypot" else name, x, n_out)
    got = dev.debug_math(pkg.DEBUG_MATH_OP[name], x)
    check(name, x, got, want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()


@pytest.fixture(scope="module")
def cstep(hm):
    """the 200000 records and the HOST's select-form output of each: the reference of every arrangement (the host's one-case form
    gives the same bits, tests/test_host_math.py::test_cstep_one_case_form_is_bitwise_the_select_form)"""
    a = math_cases.cstep_records()
    sel = np.zeros((a.shape[0], 9)); case = np.zeros((a.shape[0], 9))
    hm.hm_cstep_forms(a.shape[0], a.ctypes.data_as(hm.hm_cstep_forms.argtypes[1]), 0, sel.ctypes.data_as(hm.hm_cstep_forms.argtypes[3]),
                      case.ctypes.data_as(hm.hm_cstep_forms.argtypes[4]))
    info = sel[:, 8].astype(np.int64)
    assert all((info == c).sum() > 20 * WAVE for c in range(5)), np.bincount(info)
    return a, sel, info


def run_cstep(pkg, dev, cstep, order, label):
    a, sel, _ = cstep
    x = np.ascontiguousarray(a[order])
    check("mt_cstep, " + label, x, dev.debug_math(pkg.DEBUG_MATH_OP["mt_cstep"], x), sel[order])


def wave_view(v, order):
    """v[order] cut into full waves: (waves, 64)"""
    k = len(order) // WAVE
    return v[order[: k * WAVE]].reshape(k, WAVE)


def test_cstep_mixed_waves(pkg, dev, cstep):
    """(i) shuffled: the lanes of a wave sit in different cases (the select form); (iv) 37 records short: a ragged last wave"""
    a, sel, info = cstep
    order = np.random.default_rng(5).permutation(a.shape[0])
    w = wave_view(info, order)
    assert np.mean([len(set(r[r > 0])) > 1 for r in w]) > 0.99
    run_cstep(pkg, dev, cstep, order, "shuffled")
    assert (a.shape[0] - 37) % WAVE not in (0, 1, 63)
    run_cstep(pkg, dev, cstep, order[: a.shape[0] - 37], "shuffled, ragged last wave")


def test_cstep_one_case_waves(pkg, dev, cstep):
    """(ii) sorted by case: all the lanes of a wave that reach the selection sit in one case, the wave takes mt_cstep_case<C>; in case 4
    any_brackt comes from a ballot -- waves with no bracketing lane skip the cubic, waves with some or all evaluate it.  (iv) the same,
    37 records short."""
    a, sel, info = cstep
    order = math_cases.cstep_case_sorted(info, a[:, 11])
    assert np.array_equal(np.sort(order), np.arange(a.shape[0])) and np.all(np.diff(info[order]) >= 0)
    wi, wb = wave_view(info, order), wave_view(a[:, 11], order)
    for c in (1, 2, 3, 4):
        assert np.all(wi == c, axis=1).sum() > 20, c                          # whole waves in every case
    four = np.all(wi == 4, axis=1)
    lanes = (wb[four] != 0).sum(axis=1)
    assert (lanes == 0).sum() > 10 and ((lanes > 0) & (lanes < WAVE)).sum() > 10 and (lanes == WAVE).sum() > 10, np.bincount(lanes, minlength=WAVE + 1)
    run_cstep(pkg, dev, cstep, order, "one case per wave")
    run_cstep(pkg, dev, cstep, order[: a.shape[0] - 37], "one case per wave, ragged last wave")


def test_cstep_one_case_waves_with_lanes_that_left_at_the_guard(pkg, dev, cstep):
    """(iii) arrangement (ii) with records that fail the guard (info 0) dealt into every wave: those lanes return before the ballot, so the
    other lanes are still a one-case wave and must still agree"""
    a, sel, info = cstep
    dead = 8
    order = math_cases.cstep_with_dead_lanes(math_cases.cstep_case_sorted(info, a[:, 11]), info, dead)
    assert len(set(order.tolist())) == len(order) and len(order) % WAVE == 0
    wi, wb = wave_view(info, order), wave_view(a[:, 11], order)
    assert np.all((wi == 0).sum(axis=1) == dead)
    assert len({tuple(np.nonzero(r == 0)[0]) for r in wi}) >= WAVE // 2          # the lanes that leave move from wave to wave
    live_case = np.where(wi == 0, wi.max(axis=1, keepdims=True), wi)
    for c in (1, 2, 3, 4):
        assert np.all(live_case == c, axis=1).sum() > 20, c
    four = np.all(live_case == 4, axis=1)
    lanes = ((wb != 0) & (wi == 4))[four].sum(axis=1)
    assert (lanes == 0).sum() > 10 and ((lanes > 0) & (lanes < WAVE - dead)).sum() > 10 and (lanes == WAVE - dead).sum() > 10
    live = (info != 0).sum()
    assert (info[order] != 0).sum() > 0.9 * min(live, (info == 0).sum() // dead * (WAVE - dead))
    run_cstep(pkg, dev, cstep, order, "one case per wave, %d lanes of each wave left at the guard" % dead)


def test_hook_refuses_what_it_does_not_know(pkg, dev):
    """an op outside the table and a record of the wrong width are errors, an empty launch is not; the raw entry point refuses an op
    beyond the last one and a negative count before it touches the device"""
    assert sorted(pkg.DEBUG_MATH_OP.values()) == sorted(pkg.DEBUG_MATH_SHAPES) == list(range(10))
    with pytest.raises(KeyError):
        dev.debug_math(10, np.ones((4, 1)))
    with pytest.raises(ValueError):
        dev.debug_math(pkg.DEBUG_MATH_OP["svd3"], np.ones((4, 6)))
    with pytest.raises(ValueError):
        dev.debug_math(pkg.DEBUG_MATH_OP["sqrt_in_1_4"], np.ones(4))
    assert dev.debug_math(pkg.DEBUG_MATH_OP["svd32"], np.ones((0, 6))).shape == (0, 12)
    x = np.ones(16); y = np.zeros(32)
    p = lambda a: a.ctypes.data_as(dev.L.admm_hip_debug_math.argtypes[3])
    for op, n in ((10, 1), (-1, 1), (2, -1)):
        assert dev.L.admm_hip_debug_math(dev.h, op, n, p(x), p(y)) != 0
    assert np.all(y == 0.0)
