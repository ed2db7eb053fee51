#!/usr/bin/env python3
"""Writes tests/golden/rcp_hard_1_sqrt2.txt: doubles b in [1, sqrt 2] whose reciprocal lies next to a rounding midpoint --
the directed arguments of rcp_in_1_2 (csrc/local_math.hpp) in the range the Jacobi rotation reaches (tests/math_cases.py
rcp_hard_b; tests/test_host_math.py asserts the distance with integers, tests/test_device_math.py runs them on the device).

1 / b for b = B 2^-52 in (1, 2) has ulp 2^-53, so in half-ulps it is 2^106 / B, and a midpoint is an odd integer n.  No closed
form gives midpoints for B < 2^52.5 (the family b = 2 - k 2^-52 sits at the other end of the binade), so: draw odd n in
[2^53.5, 2^54), take B = round(2^106 / n) and keep the pair when 2^106 / B is within 2^-14 ulp of n, i.e.
|B n - 2^106| / (2 B) < 2^-14.  About one candidate in 11000 passes; the seed makes the file reproducible.  Run once:

    python tools/find_rcp_hard.py [candidates]
"""
import math
import os
import random
import sys

SEED = 20240607
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "rcp_hard_1_sqrt2.txt")


def search(candidates, seed=SEED):
    rng = random.Random(seed)
    lo = math.isqrt(1 << 107) + 1          # ceil(2^53.5)
    top = 1 << 106
    hits = {}
    for _ in range(candidates):
        n = rng.randrange(lo, 1 << 54) | 1
        B = (top + n // 2) // n
        if abs(B * n - top) << 14 < 2 * B and (1 << 52) <= B and B * B <= (1 << 105):
            hits[B] = n
    return sorted(hits.items())


def main():
    candidates = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    hits = search(candidates)
    with open(OUT, "w") as f:
        f.write("# B n (hex): b = B 2^-52 in [1, sqrt 2], 2^106 / B within 2^-14 ulp of the odd n (a rounding midpoint of 1 / b in half-ulps)\n")
        f.write("# tools/find_rcp_hard.py, seed %d, %d candidates\n" % (SEED, candidates))
        for B, n in hits:
            f.write("%x %x\n" % (B, n))
    print("%d arguments -> %s" % (len(hits), os.path.normpath(OUT)))


if __name__ == "__main__":
    main()
