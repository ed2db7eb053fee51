"""bench.py --dump-outputs: what the timed path computed in its last step (positions and velocities, float64, one row per
node) as DIR/<name>.npy, at most 64 MB in all, so that two builds can be compared output for output.  And what it runs: the
library build() made, loaded without writing to the tree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_small_outputs_whole(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    x, v = rng.normal(size=3 * 1000), rng.normal(size=3 * 1000)
    d = bench.dump_outputs(str(tmp_path / "out"), x, v)
    assert d["sampled"] is False and d["nodes"] == 1000 and sorted(os.listdir(tmp_path / "out")) == ["v.npy", "x.npy"]
    xs, vs = np.load(tmp_path / "out" / "x.npy"), np.load(tmp_path / "out" / "v.npy")
    assert xs.dtype == np.float64 and xs.shape == (1000, 3) and np.array_equal(xs.ravel(), x) and np.array_equal(vs.ravel(), v)


def test_dump_large_outputs_fixed_sample_under_the_cap(tmp_path):
    import bench
    n = 1500000                                                     # 72 MB of x and v: above the cap
    x = np.arange(3 * n, dtype=np.float64); v = -x
    runs = []
    for k in range(2):
        out = tmp_path / ("out%d" % k)
        d = bench.dump_outputs(str(out), x, v)
        assert d["sampled"] is True and d["nodes"] == n
        assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= bench.DUMP_MAX_BYTES
        runs.append({f[:-4]: np.load(out / f) for f in os.listdir(out)})
    r = runs[0]
    idx = r["node_index"].astype(np.int64)
    assert set(r) == {"x", "v", "node_index"} and all(a.dtype == np.float64 for a in r.values())
    assert np.all(np.diff(idx) > 0) and idx[-1] < n and idx.size > 1000000
    assert np.array_equal(r["x"], x.reshape(-1, 3)[idx]) and np.array_equal(r["v"], v.reshape(-1, 3)[idx])
    assert all(np.array_equal(r[k], runs[1][k]) for k in r)        # the same sample every time


def test_bench_refuses_no_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_exactly(pkg, tmp_path):
    """Two runs with the same arguments: the dumped positions are those the result line's checksum was taken from, --steps
    sets the timed steps, and the second run's outputs are bitwise the first's."""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--dims", "8", "8", "40", "--no-cpu-baseline", "--no-extras"]
    lines, dumps = [], []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append({k_: np.load(out / (k_ + ".npy")) for k_ in ("x", "v")})
    n_nodes = 9 * 9 * 41
    for L, d in zip(lines, dumps):
        assert L["steps"] == 3 and L["ms_per_step"] > 0 and L["dump_outputs"]["sampled"] is False
        assert d["x"].shape == (n_nodes, 3) and d["v"].shape == (n_nodes, 3) and d["x"].dtype == np.float64
        assert np.isfinite(d["x"]).all() and np.isfinite(d["v"]).all() and np.abs(d["v"]).max() > 0
        assert float(np.abs(d["x"].ravel()).sum()) == L["config"]["x_checksum"]
    assert np.array_equal(dumps[0]["x"], dumps[1]["x"]) and np.array_equal(dumps[0]["v"], dumps[1]["v"])


def test_side_figures_are_opt_in(monkeypatch):
    """A plain run measures the headline only; the CPU baseline, the class-API frame cost and the other configs wait for --full."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


@pytest.mark.gpu
def test_bench_full_adds_the_side_figures_after_the_same_steps(pkg):
    """The plain line holds no side figures; --full adds cpu_baseline (with the GPU on its sample), class_api and other_configs,
    and its headline comes from the same timed steps: the same positions, the same schema."""
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--dims", "8", "8", "40"]
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--cpu-dims", "4", "4", "12"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[mode] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    side = {"cpu_baseline", "class_api", "other_configs"}
    assert not side & set(plain) and side <= set(full)
    assert set(full) - side == set(plain)
    cb = full["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["value"] > 0 and cb["gpu_same_sample"]["ms_per_iter"] > 0
    assert full["class_api"]["ms_per_step"] > 0 and "error" not in full["other_configs"] and len(full["other_configs"]) == 3
    assert plain["config"]["x_checksum"] == full["config"]["x_checksum"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k


def test_up_to_date_build_writes_nothing(pkg, monkeypatch):
    """lib() calls build() on every load: with the library up to date that call must not write (no lock file, no directory),
    so that a process without write access to the tree can load it."""
    def no_write(*args, **kwargs):
        raise AssertionError("build() wrote to the tree although the library is up to date")
    monkeypatch.setattr(pkg._build.os, "makedirs", no_write)
    monkeypatch.setattr(pkg._build, "_build_locked", no_write)
    assert pkg._build.build() == pkg.LIB_PATH


def test_bench_never_compiles(tmp_path):
    """bench.py loads the library build() made; a missing one, or one older than a source, stops it with a message instead."""
    import types
    import bench
    d = tmp_path / "pkg"; (d / "csrc").mkdir(parents=True)
    (d / "__init__.py").write_text(""); src = d / "csrc" / "k.hip"; src.write_text("")
    fake = types.SimpleNamespace(__file__=str(d / "__init__.py"), build=None)
    bench.use_built_library(fake)
    with pytest.raises(SystemExit, match="build"):
        fake.build()                                   # missing
    so = d / "libadmm_hip.so"; so.write_text("")
    os.utime(src, (1e9, 1e9)); os.utime(so, (2e9, 2e9))
    assert fake.build() == str(so)                     # newer than every source
    os.utime(src, (3e9, 3e9))
    with pytest.raises(SystemExit, match="build"):
        fake.build()                                   # stale
