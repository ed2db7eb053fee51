#!/usr/bin/env python3
"""The reference's side of tests/test_oracle_vs_ref.py (needs oracle/_ref/libadmm_ref.so, i.e. the reference compiled
by oracle/Makefile): on exactly the inputs that test draws,

  * svd, corner_<kind>, project_<case>: per trial a 16-byte digest of the reference's outputs (test_oracle_vs_ref.digest);
  * assembly_*: global_idx, W and x after one ADMM iteration of the 3x3x8 StVK bar;
  * collision_*: rows, W, the collision force's global_idx and x after each of 25 frames of the floor / sphere / cylinder scene;
  * wind_x_serial / wind_x_threaded: x after each of 5 frames of the wind scene, run with 1 and with 8 OpenMP threads.

Every digest is taken twice and must agree (the reference is deterministic on these paths).
-> tests/golden/ref_pins.npz.  usage: python tests/golden/make_golden_ref_pins.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_oracle_vs_ref as T  # noqa: E402
from checkers import Ref, have_ref  # noqa: E402

assert have_ref(), "the compiled reference (oracle/_ref/libadmm_ref.so) is needed"


def twice(f, *args):
    a, b = f(Ref, *args), f(Ref, *args)
    assert np.array_equal(a, b), args
    return a


out = {}
out["svd"] = np.array([twice(T.svd_digest, F, G) for F, G in T.svd_inputs()])
for name, params in T.CORNER_CASES:
    out["corner_" + name] = np.array([twice(T.corner_digest, name, params, X, Dx) for X, Dx in T.corner_inputs(name)])
for i, (name, params) in enumerate(T.CASES):
    out["project_%d" % i] = np.array([twice(T.project_digest, name, params, x, Dx, u0) for x, Dx, u0 in T.project_inputs(name, params)])

r = T.assembly_system(Ref)
out["assembly_global_idx"], out["assembly_wdiag"] = r.global_idx(), r.wdiag
r.step()
out["assembly_x1"] = r.x

r, nt = T.collision_system(reference=True)
out["collision_rows"], out["collision_wdiag"], out["collision_last_global_idx"] = np.int64(r.rows), r.wdiag, np.int64(r.global_idx()[-1])
X = []
for f in range(T.COLLISION_FRAMES):
    r.step(); X.append(r.x)
out["collision_x"] = np.array(X)

with tempfile.TemporaryDirectory() as tmp:
    out["wind_x_serial"] = T.wind_frames("reference", 1, os.path.join(tmp, "serial.npy"))
    assert np.array_equal(out["wind_x_serial"], T.wind_frames("reference", 1, os.path.join(tmp, "serial2.npy")))
    out["wind_x_threaded"] = T.wind_frames("reference", 8, os.path.join(tmp, "threaded.npy"))

np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_pins.npz"), **out)
print("ref_pins.npz:", ", ".join("%s %s" % (k, v.shape) for k, v in out.items()))
