"""The argument sets of the per-lane math tests, seeded and shared: tests/test_host_math.py runs the HOST build of
csrc/local_math.hpp on them (and checks the sets themselves with integers), tests/test_device_math.py the DEVICE build.

The scalar helpers sqrt_in_1_4 / sqrt_ge_1 / rcp_in_1_2 claim correct rounding on a stated range.  An algorithm whose error
is 0.5 + 1e-6 ulp is wrong on one random argument in a million but on every second argument whose exact result sits next
to a rounding midpoint, so each helper gets a HARD set built with integers (exact distance to the midpoint known) next to
the millions of ordinary arguments.  No set holds an argument outside a helper's stated range: the range is its contract.

Every set is generated once per process (functools.lru_cache) and must not be written to."""
import functools
import math
import os

import numpy as np

from checkers import extreme_matrices

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
SQRT2 = math.sqrt(2.0)


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def _bits(v):
    return int(np.float64(v).view(np.int64))


def _from_bits(b):
    return np.asarray(b, dtype=np.int64).view(np.float64)


def neighbours(v, below, above):
    """the doubles from `below` steps under the positive double v to `above` steps over it, v included"""
    return _from_bits(_bits(v) + np.arange(-below, above + 1, dtype=np.int64))


def nans():
    """quiet and signalling, both signs, several payloads"""
    return np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001, 0x7fffffffffffffff, 0x7ff0000000000001, 0xfff4000000000000,
                     0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)


# ---- exact references with Python integers ------------------------------------------------------------------------------
def _mant(x):
    """a positive finite double as (M, e): x == M * 2**e, M an integer below 2**53"""
    m, e = math.frexp(x)
    return int(math.ldexp(m, 53)), e - 53


def exact_sqrt(x):
    """the correctly rounded square root of a positive finite double, computed with integers"""
    M, e = _mant(float(x))
    s = 108 - M.bit_length()
    if (e - s) & 1:
        s -= 1
    q = math.isqrt(M << s)            # M << s in [2^106, 2^108): q = floor(root) has 54 bits, the last one is the rounding bit
    # q even: the root lies in [q, q + 1), under the midpoint q + 1.  q odd: it lies over the midpoint q (it cannot BE q: q * q is odd,
    # M << s is not, s being positive for a 53-bit M) -- round up
    r = (q + 1) >> 1
    return math.ldexp(r, (e - s) // 2 + 1)


def exact_rcp(b):
    """the correctly rounded 1 / b of a positive finite double (ties to even), computed with integers"""
    M, e = _mant(float(b))            # M in [2^52, 2^53): 2^105 / M in (2^52, 2^53] -- 53 bits and the remainder
    q, rem = divmod(1 << 105, M)
    if 2 * rem > M or (2 * rem == M and (q & 1)):
        q += 1
    return math.ldexp(q, -e - 105)


# ---- square root: the hard set ----------------------------------------------------------------------------------------------
def _sqrt_mod_pow2(r, K):
    """the four solutions of n^2 = r (mod 2^K) for r = 1 (mod 8), by Hensel lifting"""
    s = 1
    for j in range(3, K):            # s^2 = r (mod 2^j); (s + 2^(j-1))^2 = s^2 + 2^j (mod 2^(j+1)) for odd s
        if (s * s - r) >> j & 1:
            s += 1 << (j - 1)
    M = 1 << K
    return sorted({s % M, -s % M, (s + M // 2) % M, (M // 2 - s) % M})


@functools.lru_cache(None)
def sqrt_hard_triples(rmax=24000):
    """(X, K, n): x = X 2^(K-106) is a double in [1, 4) (K = 54: [1, 2), K = 55: [2, 4)), n is odd, and n^2 - X 2^K = r with |r| < rmax.
    The root of x in half-ulps is sqrt(X 2^K) = n - r / (2 n) + ...: within |r| / (4 n) ulp of the rounding midpoint n."""
    out = []
    for r in range(-rmax + 1, rmax):
        if r % 8 != 1:
            continue
        for K in (54, 55):
            for n in _sqrt_mod_pow2(r, K):
                if not (1 << 53) <= n < (1 << 54):
                    continue
                X = (n * n - r) >> K
                if (1 << 52) <= X < (1 << 53):
                    out.append((X, K, n))
    return tuple(sorted(set(out)))


@functools.lru_cache(None)
def sqrt_hard():
    """doubles in [1, 4) whose exact root lies within 1.4e-12 ulp of a rounding midpoint"""
    return _frozen(sorted({math.ldexp(X, K - 106) for X, K, n in sqrt_hard_triples()}))


# ---- square root: everything ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sqrt_in_1_4_args():
    """sqrt_in_1_4: x in [1, 4) or NaN.  The hard set comes first (the short launches n = 1, 63, 64, 65 are prefixes)."""
    rng = np.random.default_rng(1404)
    k = rng.integers(2 ** 25, 2 ** 26, 100_000).astype(np.float64) * 2.0 ** -25         # m in [1, 2) with 26 bits: m * m is exact
    sq = k * k
    q, p = np.abs(rng.normal(size=200_000)), np.abs(rng.normal(size=200_000))
    q, p = np.minimum(q, p), np.maximum(q, p)
    qp = np.concatenate([q / p, 10.0 ** rng.uniform(-324, 0, 100_000), rng.uniform(0, 1, 100_000),
                         [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1.0], neighbours(2.0 ** -27, 3, 3), neighbours(2.0 ** -26, 3, 3),
                         neighbours(2.0 ** -26.5, 3, 3), neighbours(1.0, 50, 0)])
    tt = np.concatenate([rng.uniform(-1, 1, 150_000), rng.choice([-1.0, 1.0], 50_000) * 10.0 ** rng.uniform(-20, 0, 50_000), [0.0, -0.0, 1.0, -1.0]])
    x = np.concatenate([
        sqrt_hard(),
        rng.uniform(1, 4, 1_100_000),
        _from_bits(rng.integers(_bits(1.0), _bits(4.0), 200_000)),                      # uniform in the bits: both binades alike
        neighbours(1.0, 0, 1000), neighbours(2.0, 1000, 1000), neighbours(4.0, 1000, -1),
        sq, _from_bits(sq.view(np.int64) + 1), _from_bits(sq.view(np.int64) - 1),
        1.0 + qp * qp, tt * tt + 1.0,                                                  # makeJacobi / numext::hypot as jacobi_pq forms them
        nans()])
    ok = np.isnan(x) | ((x >= 1.0) & (x < 4.0))
    return _frozen(x[ok])


@functools.lru_cache(None)
def sqrt_ge_1_args():
    """sqrt_ge_1: x in [1, +inf] or NaN"""
    rng = np.random.default_rng(1405)
    tau = np.concatenate([10.0 ** rng.uniform(-200, 200, 150_000), 10.0 ** rng.uniform(-3, 3, 50_000), rng.normal(size=50_000)])
    p2 = 2.0 ** np.arange(0, 1024)
    with np.errstate(over="ignore"):
        x = np.concatenate([
            sqrt_in_1_4_args(),
            tau * tau + 1.0,                                                           # overflows to +inf from |tau| = 1.4e154 on
            p2, _from_bits(p2.view(np.int64) + 1), _from_bits(p2.view(np.int64)[1:] - 1),
            _from_bits(rng.integers(_bits(1.0), _bits(np.finfo(np.float64).max), 200_000)),      # any exponent, any mantissa
            [np.finfo(np.float64).max, np.inf], nans()])
    assert np.all(np.isnan(x) | (x >= 1.0))
    return _frozen(x)


# ---- reciprocal -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def rcp_hard_a_pairs():
    """(B, n): b = B 2^-52 = 2 - k 2^-52 for odd k < 2^13; (2^53 - k)(2^53 + k) = 2^106 - k^2, so 2^106 / B (1 / b in half-ulps) lies
    k^2 / B above the odd n = 2^53 + k"""
    return tuple(((1 << 53) - k, (1 << 53) + k) for k in range(1, 1 << 13, 2))


@functools.lru_cache(None)
def rcp_hard_b_pairs():
    """(B, n) of tests/golden/rcp_hard_1_sqrt2.txt (tools/find_rcp_hard.py): b = B 2^-52 in [1, sqrt 2], the range the Jacobi
    rotation's 1 / sqrt(t^2 + 1) reaches"""
    pairs = []
    with open(os.path.join(GOLDEN, "rcp_hard_1_sqrt2.txt")) as f:
        for line in f:
            if not line.startswith("#"):
                B, n = line.split()
                pairs.append((int(B, 16), int(n, 16)))
    return tuple(pairs)


@functools.lru_cache(None)
def rcp_hard():
    """both hard sets as doubles, (a) then (b)"""
    return _frozen([math.ldexp(B, -52) for B, n in rcp_hard_a_pairs() + rcp_hard_b_pairs()])


@functools.lru_cache(None)
def rcp_in_1_2_args():
    """rcp_in_1_2: b in [1, 2) or NaN; the hard sets first"""
    rng = np.random.default_rng(1406)
    roots = np.sqrt(np.concatenate([sqrt_hard(), sqrt_in_1_4_args()[::4]]))            # correctly rounded roots: what jacobi_pq hands over
    b = np.concatenate([
        rcp_hard(),
        rng.uniform(1, 2, 1_100_000), rng.uniform(1, SQRT2, 300_000),
        neighbours(1.0, 0, 1000), neighbours(SQRT2, 1000, 1000), neighbours(2.0, 1000, -1),
        roots, nans()])
    ok = np.isnan(b) | ((b >= 1.0) & (b < 2.0))
    return _frozen(b[ok])


# ---- eig_hypot ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def hypot_pairs(n=1_000_000):
    """(x, y) of numext::hypot as real_2x2_jacobi_svd calls it (t = m00 + m11, d = m10 - m01) and at the corners: zeros, equal
    magnitudes, denormals, huge ratios, the ends of the exponent range, inf and NaN"""
    rng = np.random.default_rng(1407)
    F = np.eye(3).reshape(1, 9) + rng.uniform(0, 1, (400_000, 1)) * rng.normal(size=(400_000, 9))
    parts = [np.stack([F[:, 0] + F[:, 4], F[:, 1] - F[:, 3]], axis=1),
             rng.normal(size=(250_000, 2)) * 10.0 ** rng.uniform(-300, 300, (250_000, 1)),
             rng.normal(size=(150_000, 2)) * 10.0 ** rng.uniform(-320, 300, (150_000, 2))]
    with np.errstate(over="ignore"):
        e = rng.normal(size=50_000) * 10.0 ** rng.uniform(-320, 308, 50_000)
    parts.append(np.stack([e, e * rng.choice([-1.0, 1.0], e.size)], axis=1))
    sp = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1.0, -1.0, 2.0 ** -27, 2.0 ** -26, 3.0, 4.0, 1e154, 1e155, 1e300,
                   1.7976931348623157e308, np.inf, -np.inf, np.nan])
    parts.append(np.array([(a, b) for a in sp for b in sp]))
    k = n - sum(len(p) for p in parts)
    z = rng.normal(size=(k, 2)); z[rng.uniform(size=k) < 0.5, 0] = 0.0; z[rng.uniform(size=k) < 0.1, 1] = 0.0
    parts.append(z)
    return _frozen(np.concatenate(parts))


# ---- matrices -----------------------------------------------------------------------------------------------------------------
def _rotations(rng, n):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b, c, d = q.T
    R = np.empty((n, 3, 3))
    R[:, 0, 0] = a * a + b * b - c * c - d * d; R[:, 0, 1] = 2 * (b * c - a * d); R[:, 0, 2] = 2 * (b * d + a * c)
    R[:, 1, 0] = 2 * (b * c + a * d); R[:, 1, 1] = a * a - b * b + c * c - d * d; R[:, 1, 2] = 2 * (c * d - a * b)
    R[:, 2, 0] = 2 * (b * d - a * c); R[:, 2, 1] = 2 * (c * d + a * b); R[:, 2, 2] = a * a - b * b - c * c + d * d
    return R


def _threshold_blocks(rng, per):
    """diagonal matrices with ONE pair (p, q) coupled by off-diagonals at f * 2 eps max(|d_p|, |d_q|), f = 1, 2, 4 -- jacobi_pq rotates when
    an off-diagonal EXCEEDS 2 eps max|diag| -- the threshold itself and two doubles to either side, on one side of the diagonal, on the
    other, on both with equal and with opposite signs.  Half the diagonals have 1 as their largest entry (svd3's scaling is then exact)."""
    out = []
    for p, q in ((1, 0), (2, 0), (2, 1)):
        for f in (1.0, 2.0, 4.0):
            for step in (-2, -1, 0, 1, 2):
                for place in range(4):
                    d = rng.uniform(0.1, 1.0, (per, 3)) * rng.choice([-1.0, 1.0], (per, 3))
                    d[: per // 2, rng.integers(0, 3)] = 1.0
                    d[per // 2:] *= 10.0 ** rng.integers(-3, 4, (per - per // 2, 1))
                    off = _from_bits((f * 2.0 * EPS * np.maximum(np.abs(d[:, p]), np.abs(d[:, q]))).view(np.int64) + step)
                    A = np.zeros((per, 9))
                    A[:, 0] = d[:, 0]; A[:, 4] = d[:, 1]; A[:, 8] = d[:, 2]
                    if place in (0, 2, 3): A[:, p + 3 * q] = off                      # column-major: (row, col) at row + 3 col
                    if place in (1, 2): A[:, q + 3 * p] = off
                    if place == 3: A[:, q + 3 * p] = -off
                    out.append(A)
    return np.concatenate(out)


@functools.lru_cache(None)
def svd3_structured():
    """the matrices that walk svd3's corners (column-major 9-vectors): checkers.extreme_matrices over 50 seeds, rank 0 / 1 / 2, repeated
    singular values, reflections, 2x2 blocks at the Jacobi threshold"""
    rng = np.random.default_rng(1408)
    parts = [np.concatenate([extreme_matrices(np.random.default_rng(1000 + s), 200) for s in range(50)])]
    k = 3000
    a, b, c, d = (rng.normal(size=(k, 3)) for _ in range(4))
    r1 = (a[:, :, None] * b[:, None, :]).reshape(k, 9) * 10.0 ** rng.integers(-3, 4, (k, 1))
    r2 = r1 + (c[:, :, None] * d[:, None, :]).reshape(k, 9)
    parts += [np.zeros((4, 9)), r1, r2]
    # repeated singular values: exactly (diagonal, permuted, signed) and to rounding (rotated)
    s = rng.uniform(0.2, 3.0, (k, 2))
    sv = np.stack([s[:, 0], s[:, 0], s[:, 1]], axis=1)
    sv[k // 3: 2 * k // 3, 1] = s[k // 3: 2 * k // 3, 1]; sv[2 * k // 3:, 2] = s[2 * k // 3:, 0]      # (a a b), (a b b), (a a a)
    D = np.zeros((k, 3, 3)); D[:, [0, 1, 2], [0, 1, 2]] = sv
    P = np.eye(3)[[rng.permutation(3) for _ in range(k)]]
    parts += [(P @ D * rng.choice([-1.0, 1.0], (k, 1, 3))).reshape(k, 9), (_rotations(rng, k) @ D @ _rotations(rng, k).transpose(0, 2, 1)).reshape(k, 9)]
    # reflections: det < 0 through one negative singular direction, -R, mirrored near-identities
    sv = rng.uniform(0.2, 3.0, (k, 3)); sv[:, 2] *= -1.0
    D = np.zeros((k, 3, 3)); D[:, [0, 1, 2], [0, 1, 2]] = sv
    M = np.eye(3).reshape(1, 9) + 0.3 * rng.normal(size=(k, 9)); M[:, 6:9] *= -1.0
    parts += [(_rotations(rng, k) @ D @ _rotations(rng, k).transpose(0, 2, 1)).reshape(k, 9), -_rotations(rng, k).reshape(k, 9), M]
    parts.append(_threshold_blocks(rng, 80))
    return _frozen(np.concatenate(parts))


@functools.lru_cache(None)
def svd3_matrices(n=1_000_000):
    """svd3 / oriented_svd records: svd3_structured(), then identity + amp * normal with amp from 0 to 1 (what a simulation produces) and
    normal matrices at every power of ten from 1e-300 to 1e300"""
    rng = np.random.default_rng(1409)
    S = svd3_structured()
    k10 = 100_000
    k = n - len(S) - k10
    amp = rng.uniform(0, 1, (k, 1)); amp[::64] = 0.0; amp[1::64] = 1.0; amp[2::64] = 10.0 ** rng.uniform(-17, -1, (len(amp[2::64]), 1))
    near = np.eye(3).reshape(1, 9) + amp * rng.normal(size=(k, 9))
    p10 = rng.normal(size=(k10, 9)) * 10.0 ** rng.integers(-300, 301, (k10, 1))
    return _frozen(np.concatenate([S, near, p10]))


@functools.lru_cache(None)
def svd32_structured():
    """3x2 (column-major 6-vectors): svd3_structured() cut to two columns, the zero Householder tails (column 0 = (a, 0, 0); the second
    reflector's tail b2 = 0) and the rank-one / zero-column cases of test_svd32"""
    rng = np.random.default_rng(1410)
    k = 3000
    F = [np.array(svd3_structured()[:, :6])]
    A = rng.normal(size=(k, 6)) * 10.0 ** rng.integers(-3, 4, (k, 1)); A[:, 1:3] = 0.0; F.append(A)                  # zero tail of Householder 0
    A = rng.normal(size=(k, 6)); A[:, 1:3] = 0.0; A[:, 5] = 0.0; F.append(A)                                        # ... and of Householder 1
    A = rng.normal(size=(k, 6)); A[:, 2] = 0.0; A[:, 5] = 0.0; F.append(A)                                          # a flat triangle: third row zero
    A = rng.normal(size=(k, 6)); A[:, 3:6] = A[:, 0:3] * rng.choice([1.0, -2.0, 0.5, 1e-8], (k, 1)); F.append(A)     # rank one
    A = rng.normal(size=(k, 6)); A[:, 3:6] = 0.0; F.append(A)
    A = rng.normal(size=(k, 6)); A[:, 0:3] = 0.0; F.append(A)
    A = rng.normal(size=(k, 6)); A[:, 3:6] = A[:, [1, 0, 2]] * np.array([[-1.0, 1.0, 0.0]]); A[:, 2] = 0.0; F.append(A)   # equal norms, orthogonal columns
    F.append(np.zeros((4, 6)))
    return _frozen(np.concatenate(F))


@functools.lru_cache(None)
def svd32_matrices(n=1_000_000):
    rng = np.random.default_rng(1411)
    S = svd32_structured()
    k10 = 100_000
    k = n - len(S) - k10
    amp = rng.uniform(0, 1, (k, 1)); amp[::64] = 0.0; amp[1::64] = 1.0
    near = np.eye(3)[:, :2].ravel(order="F").reshape(1, 6) + amp * rng.normal(size=(k, 6))
    p10 = rng.normal(size=(k10, 6)) * 10.0 ** rng.integers(-300, 301, (k10, 1))
    return _frozen(np.concatenate([S, near, p10]))


# ---- MoreThuente::cstep records -------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cstep_records():
    """200000 x [stx fx dx sty fy dy stp fp dp stpmin stpmax brackt] (tests/host_math_shim.cpp hm_cstep_forms): every case with and without a
    bracket, and the degenerate inputs (equal points, zero slopes, infinities) where the cubic produces NaN"""
    rng = np.random.default_rng(77)
    n = 200000
    a = np.zeros((n, 12))
    stx = rng.uniform(0, 2, n) * rng.choice([0, 1, 1, 1], n)
    stp = stx + rng.choice([-1, 1, 1, 1], n) * 10 ** rng.uniform(-6, 1, n)
    sty = np.where(rng.uniform(size=n) < 0.5, stx, stx + rng.choice([-1, 1], n) * 10 ** rng.uniform(-6, 1, n))
    fx = rng.normal(size=n) * 10 ** rng.uniform(-2, 4, n)
    a[:, 0] = stx; a[:, 1] = fx
    a[:, 2] = -np.sign(stp - stx) * 10 ** rng.uniform(-8, 4, n)                 # a descent direction seen from stx
    a[:, 3] = sty; a[:, 4] = fx + rng.normal(size=n) * 10 ** rng.uniform(-6, 2, n); a[:, 5] = rng.normal(size=n) * 10 ** rng.uniform(-8, 4, n)
    a[:, 6] = stp
    a[:, 7] = fx + rng.normal(size=n) * 10 ** rng.uniform(-8, 2, n)
    a[:, 8] = rng.normal(size=n) * 10 ** rng.uniform(-8, 4, n)
    br = rng.uniform(size=n) < 0.5
    a[:, 11] = br
    a[:, 9] = np.where(br, np.minimum(stx, sty) - 1e-3, stx); a[:, 10] = np.where(br, np.maximum(stx, sty) + 10, stp + 4 * (stp - stx))
    k = np.arange(n)
    a[k % 97 == 0, 8] = 0.0; a[k % 89 == 0, 2] *= 0; a[k % 83 == 0, 7] = a[k % 83 == 0, 1]      # zero slopes, equal values
    a[k % 79 == 0, 8] = a[k % 79 == 0, 2]; a[k % 73 == 0, 8] = -a[k % 73 == 0, 2]
    a[k % 71 == 0, 7] = np.inf; a[k % 67 == 0, 8] = np.inf; a[k % 61 == 0, 7] = np.nan
    a[k % 59 == 0, 3] = a[k % 59 == 0, 6]                                                        # sty == stp: 0 / 0 in case 4
    return _frozen(a)


WAVE = 64


def cstep_case_sorted(info, brackt):
    """order of the records sorted by the step selection's case (the host's info, 0 = left at the guard), so that a wave of 64 holds one
    case and takes mt_cstep_case<C>.  Equal cases keep their order, except that case 4 is laid out as [no bracket | alternating |
    bracket]: its waves then come in the three kinds the any_brackt ballot tells apart -- none, some, all lanes bracketed."""
    order = np.argsort(info, kind="stable")
    four = order[info[order] == 4]
    nb, b = four[brackt[four] == 0], four[brackt[four] != 0]
    h_nb, h_b = len(nb) // 2, len(b) // 2
    m = min(len(nb) - h_nb, h_b)
    mixed = np.empty(2 * m, dtype=order.dtype); mixed[0::2] = nb[h_nb: h_nb + m]; mixed[1::2] = b[:m]
    laid = np.concatenate([nb[:h_nb], nb[h_nb + m:], mixed, b[m:]])
    assert len(laid) == len(four)
    order = order.copy()
    order[info[order] == 4] = laid
    return order


def cstep_with_dead_lanes(order, info, dead_per_wave=8):
    """`order` (cstep_case_sorted) with records that fail the guard (info 0) dealt into every wave: each wave of 64 holds
    dead_per_wave of them, at lane positions that move from wave to wave, the other lanes keep the sorted live records"""
    dead, live = order[info[order] == 0], order[info[order] != 0]
    per = WAVE - dead_per_wave
    n_waves = min(len(dead) // dead_per_wave, len(live) // per)
    out = np.empty(n_waves * WAVE, dtype=order.dtype)
    lane = np.arange(WAVE)
    for w in range(n_waves):
        is_dead = ((lane * 5 + w) % WAVE) < dead_per_wave          # 5 is coprime to 64: dead_per_wave distinct lanes, another set per wave
        seg = out[w * WAVE: (w + 1) * WAVE]
        seg[is_dead] = dead[w * dead_per_wave: (w + 1) * dead_per_wave]
        seg[~is_dead] = live[w * per: (w + 1) * per]
    return out
