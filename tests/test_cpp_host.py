"""The C++ host-side mirror of the reference's class API
(admm-elastic-sca_amd/host/admm/*.hpp over the C ABI): the reference's two
sample programs and a ForceBuilder-style scene, compiled with g++ against the
mirror and libadmm_hip.so.  CPU: they compile, link and fail loudly without a
GPU.  GPU: known answers and parity with the oracle."""
import os
import time
import struct
import subprocess

import numpy as np
import pytest

from checkers import KIND, Oracle
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "admm-elastic-sca_amd")
BUILD = os.path.join(ROOT, "tests", "_build")


def compile_cpp(name, pkg):
    pkg.lib()
    os.makedirs(BUILD, exist_ok=True)
    extra = os.environ.get("ADMM_TEST_CXXFLAGS", "").split()      # tools/asan_host.sh: -fsanitize=address,undefined for the header-only host classes
    out = os.path.join(BUILD, name + ("_san" if extra else ""))
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-DADMM_HOST_NO_EIGEN"] + extra + [ "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(PKG, "host", "admm"), "-I" + os.path.join(ROOT, "include"), src, "-o", out,
           "-L" + PKG, "-ladmm_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return out


def have_gpu():
    import torch
    return torch.cuda.is_available()


def test_compiles_and_fails_loudly_without_gpu(pkg):
    for name in ("singletet", "singlenode", "scene_bar", "scene_ranks", "scene_plinko", "user_force", "dillo_main"):
        exe = compile_cpp(name, pkg)
        assert os.path.exists(exe)
    if have_gpu():
        pytest.skip("GPU present: behaviour covered by the gpu tests")
    r = subprocess.run([os.path.join(BUILD, "singletet")], capture_output=True, text=True)
    assert r.returncode == 2                       # initialize() returned false
    assert "no usable HIP device" in r.stderr or "no HIP device" in r.stderr


@pytest.mark.gpu
def test_singletet_singlenode(pkg):
    g = golden("known_answers.npz")
    r = subprocess.run([compile_cpp("singletet", pkg)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Node 4 x: 171.571" in r.stdout          # the reference's printed answer
    full = [float(v) for v in r.stdout.split("full:")[1].split()]
    assert abs(full[0] - 171.57142857142716) < 1e-9 and np.abs(np.array(full) - g["singletet_x"][9:12]).max() < 1e-9
    r = subprocess.run([compile_cpp("singlenode", pkg)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("step:")]
    assert [l.split("pos: ")[1] for l in lines] == ["(0, -9.8, 0)", "(0, -29.4, 0)", "(0, -58.8, 0)", "(0, -98, 0)"]


@pytest.mark.gpu
@pytest.mark.parametrize("typ", [0, 1])
def test_scene_through_class_api(pkg, tmp_path, typ):
    mg = pkg.meshgen
    dims = (3, 3, 8)
    x, t = mg.bar(*dims)
    m = mg.lumped_tet_mass(x, t, 1000.0)
    anchors = mg.bar_anchor_nodes(dims[0], dims[1])
    moving = x.shape[0] - 1
    inp = tmp_path / "in.bin"; outp = tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("4i", x.shape[0], t.shape[0], anchors.size, typ))
        f.write(x.astype(np.float64).tobytes()); f.write(np.repeat(m, 3).tobytes()); f.write(t.astype(np.int32).tobytes())
        f.write(anchors.astype(np.int32).tobytes()); f.write(struct.pack("i", moving))
    frames, iters = 6, 10
    r = subprocess.run([compile_cpp("scene_bar", pkg), str(inp), str(outp), str(frames), str(iters)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = np.fromfile(outp, dtype=np.float64)
    n3 = 3 * x.shape[0]
    X = raw[:frames * n3].reshape(frames, n3)
    nf = t.shape[0] + anchors.size + 1
    meta = raw[frames * n3:frames * n3 + 2 * nf].reshape(nf, 2)
    cp_final = raw[-3:]
    # the same scene on the oracle, control point scripted identically
    o = Oracle(); o.settings(0.04, iters)
    o.add_nodes(x.ravel(), np.repeat(m, 3))
    o.add_forces(KIND["TET_STVK" if typ else "TET_NH"], t, [1e5, 1e5, 5])
    o.add_forces(KIND["ANCHOR"], anchors, [-1.0, 1.0])
    start = x[moving].copy(); end = start + np.array([0, 0.05, 0])
    h = o.add_moving_anchor(moving, start, True, -1.0)
    o.add_gravity([0, -9.8, 0])
    assert o.initialize()
    assert np.array_equal(meta[:, 0].astype(np.int64), o.global_idx())       # element indexing
    assert np.array_equal(meta[:, 1], o.weights())                           # weights bit-exact
    elapsed = 0.0
    for fr in range(frames):
        tr = elapsed / 0.2
        pos = start if elapsed < 0 else (end if tr > 1 else start + (3 * tr * tr - 2 * tr ** 3) * (end - start))
        active = fr < 3
        if active:
            o.set_control_point(h, pos, True)
        else:
            o.set_control_point(h, np.array(list(o.force(h).pos)), False)
        o.step(); elapsed += 0.04
        assert np.abs(X[fr] - o.x).max() < 2e-4, fr       # within the truncated-prox sensitivity
    assert np.abs(cp_final - np.array(list(o.force(h).pos))).max() < 2e-4


def test_shard_from_env(pkg):
    """System::shard.from_env() reads what torchrun / Open MPI / Slurm export (the C++ host's way to one process per GPU)."""
    exe = compile_cpp("shard_env", pkg)
    clean = {k: v for k, v in os.environ.items() if not any(k.startswith(p) for p in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "OMPI_", "SLURM_", "MASTER_", "ADMM_HIP_RCCL"))}

    def run(**env):
        return subprocess.run([exe], capture_output=True, text=True, env=dict(clean, **env), timeout=60).stdout.strip()
    assert run() == "local -1 rank 0 world 1 file"
    out = run(RANK="3", WORLD_SIZE="8", LOCAL_RANK="3", MASTER_PORT="29511")
    assert out.startswith("local 3 rank 3 world 8 file /tmp/admm_hip_rccl_id.") and out.endswith(".29511")
    assert run(OMPI_COMM_WORLD_RANK="5", OMPI_COMM_WORLD_SIZE="16", OMPI_COMM_WORLD_LOCAL_RANK="1", ADMM_HIP_RCCL_ID_FILE="/shared/job7.id") == "local 1 rank 5 world 16 file /shared/job7.id"
    assert run(SLURM_PROCID="2", SLURM_NTASKS="4", SLURM_LOCALID="2", SLURM_JOB_ID="991").endswith(".991")
    # nothing job-unique in the environment: no default name two jobs could share (initialize() then asks for ADMM_HIP_RCCL_ID_FILE)
    assert run(RANK="1", WORLD_SIZE="2", LOCAL_RANK="1") == "local 1 rank 1 world 2 file"


def test_comm_helpers_on_the_cpu(pkg, tmp_path):
    """host/admm/Comm.hpp without a GPU: the shared-memory all-reduce between three processes (every rank gets the sum added
    in rank order, bit for bit, also when the buffer needs several rounds through the segment) and the rendezvous file that
    carries the RCCL id from rank 0 to the others (atomic publish, waiting reader, leftovers of earlier jobs ignored)."""
    exe = compile_cpp("comm_check", pkg)
    name = "/admm_comm_check_%d" % os.getpid()
    ps = [subprocess.Popen([exe, "shm", name, str(r), "3", "5000", "1024"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(3)]
    outs = [p.communicate(timeout=120) for p in ps]
    assert all(p.returncode == 0 for p in ps), outs
    assert len({o[0] for o in outs}) == 1 and outs[0][0].startswith("ok ")
    idf = str(tmp_path / "rccl_id")
    reader = subprocess.Popen([exe, "file", idf, "1"], stdout=subprocess.PIPE, text=True)          # waits for rank 0
    writer = subprocess.run([exe, "file", idf, "0"], capture_output=True, text=True, timeout=60)
    assert writer.returncode == 0 and reader.communicate(timeout=60)[0] == writer.stdout and writer.stdout.startswith("ok ")
    old = os.path.getmtime(idf) - 7200
    os.utime(idf, (old, old))                                                                    # a leftover of an earlier job
    stale = subprocess.run([exe, "file", idf, "1", "600"], capture_output=True, text=True, timeout=60)
    assert stale.returncode == 5 and "timed out" in stale.stdout
    # the id of ANOTHER launch (other port -> other nonce in the file) is not taken, however fresh
    idf2 = str(tmp_path / "rccl_id2")
    env_a, env_b = dict(os.environ, MASTER_PORT="29611"), dict(os.environ, MASTER_PORT="29612")
    assert subprocess.run([exe, "file", idf2, "0"], capture_output=True, text=True, timeout=60, env=env_a).returncode == 0
    other = subprocess.run([exe, "file", idf2, "1"], capture_output=True, text=True, timeout=60, env=env_b)
    assert other.returncode == 5 and "timed out" in other.stdout
    assert subprocess.run([exe, "file", idf2, "1"], capture_output=True, text=True, timeout=60, env=env_a).stdout.startswith("ok ")
    # a symlink under the name is not followed by the reader, and rank 0 replaces it instead of writing through it
    victim = tmp_path / "victim"; victim.write_bytes(b"x" * 144)
    idf3 = str(tmp_path / "rccl_id3"); os.symlink(str(victim), idf3)
    assert subprocess.run([exe, "file", idf3, "1"], capture_output=True, text=True, timeout=60).returncode == 5
    assert subprocess.run([exe, "file", idf3, "0"], capture_output=True, text=True, timeout=60).returncode == 0
    assert victim.read_bytes() == b"x" * 144 and not os.path.islink(idf3) and oct(os.stat(idf3).st_mode & 0o777) == "0o600"
    # the same ShmAllReduce object opened again after close(): the barrier's sense starts over
    ps = [subprocess.Popen([exe, "reopen", name + "_re", str(r), "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=120) for p in ps]
    assert all(p.returncode == 0 for p in ps), outs
    # a crashed run's segment left under the name: a rank that attaches to it before rank 0 has replaced it finds its way to the new one
    import mmap, struct
    seg = "/dev/shm" + name + "_stale"
    nbytes = 64 + 8 * 1024 * 2
    with open(seg, "wb") as f:
        f.write(struct.pack("<IiiiI", 0xADB17E55, 0, 0, 0, 2).ljust(64, b"\0")); f.truncate(nbytes)
    late = subprocess.Popen([exe, "shm", name + "_stale", "1", "2", "100", "1024"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    time.sleep(0.5)                                                                              # rank 1 now sits on the orphan's barrier
    first = subprocess.Popen([exe, "shm", name + "_stale", "0", "2", "100", "1024"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    o0, o1 = first.communicate(timeout=120), late.communicate(timeout=120)
    assert first.returncode == 0 and late.returncode == 0 and o0[0] == o1[0], (o0, o1)


MAX_RANK_PROCS = 4      # processes that open the GPU at once, besides the test's own: a shared GPU node allows six in all


@pytest.mark.gpu
@pytest.mark.parametrize("world,mode", [(2, 1), (3, 1), (2, 0), (4, 1), (8, 1)])
def test_scene_through_class_api_multi_rank(pkg, tmp_path, monkeypatch, world, mode):
    """Multi-GPU from the C++ class API (System::shard; System.hpp:29-76 has no counterpart -- the reference's element loop is
    one OpenMP team, System.cpp:57-58): `world` ranks each build the whole scene of scene_bar.cpp and own a shard of its
    elements (mode 1: elimination subtrees, 0: contiguous ranges); on this one-GPU box they share the GPU and meet in
    comm::ShmAllReduce instead of RCCL.  Up to 4 ranks are 4 processes; 8 ranks are 4 processes of two ranks each (one host
    thread and one System per rank).  Every rank ends every frame with the complete, identical m_x, equal to the
    single-process run up to the order of the partial sums."""
    mg = pkg.meshgen
    if world >= 4:
        monkeypatch.setenv("ADMM_HIP_DIST_TOP", "1")      # the distributed top (two collectives per iteration) through the class API; by default only from 300k nodes on
    dims = (8, 8, 40) if world < 4 else (12, 12, 60)      # 3321 nodes: beyond the explicit-inverse solve, so the subtree split is real; 4 / 8 ranks (round 6: what the first
    x, t = mg.bar(*dims)                                   # multi-GPU run starts -- 8 real processes, rank-local factorization, a top of several levels): 10 309 nodes
    m = mg.lumped_tet_mass(x, t, 1000.0)
    anchors = mg.bar_anchor_nodes(dims[0], dims[1])
    moving = x.shape[0] - 1
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("4i", x.shape[0], t.shape[0], anchors.size, 1))       # StVK
        f.write(x.astype(np.float64).tobytes()); f.write(np.repeat(m, 3).tobytes()); f.write(t.astype(np.int32).tobytes())
        f.write(anchors.astype(np.int32).tobytes()); f.write(struct.pack("i", moving))
    exe = compile_cpp("scene_ranks", pkg)
    n3 = 3 * x.shape[0]

    def run(frames, iters, tag):
        def load(path):
            raw = np.fromfile(path, dtype=np.float64)
            return raw[:frames * n3].reshape(frames, n3), raw[-3:]
        one = tmp_path / (tag + "one.bin")
        r = subprocess.run([exe, str(inp), str(one), str(frames), str(iters), "0", "1", "1"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        name = "/admm_scene_ranks_%d_%d%d%s" % (os.getpid(), world, mode, tag)
        outs = [tmp_path / ("%srank%d.bin" % (tag, k)) for k in range(world)]
        # at most MAX_RANK_PROCS processes on the GPU besides this one: process p hosts ranks p, p + nproc, ... (one host thread each)
        nproc = min(world, MAX_RANK_PROCS)
        ps = [subprocess.Popen([exe, str(inp), ",".join(str(outs[k]) for k in range(p, world, nproc)), str(frames), str(iters),
                                ",".join(str(k) for k in range(p, world, nproc)), str(world), str(mode), name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
              for p in range(nproc)]
        res = [p.communicate(timeout=600) for p in ps]
        assert all(p.returncode == 0 for p in ps), res
        Xs = [load(o) for o in outs]
        for k in range(1, world):            # replicated top / all-reduced right-hand side: every rank holds the same bits
            assert np.array_equal(Xs[k][0], Xs[0][0]) and np.array_equal(Xs[k][1], Xs[0][1])
        assert np.isfinite(Xs[0][0]).all()
        return load(one), Xs[0]
    # one ADMM iteration per frame: the partial sums meet in another order, nothing else differs -> rounding level
    (X1, _), (Xw, _) = run(2, 1, "a")
    assert np.abs(Xw[0] - X1[0]).max() < 1e-11
    # ten iterations per frame, five frames: the truncated StVK prox amplifies last-bit differences of its input (the reference
    # against itself from a 1-ulp perturbed start: 2e-6 after one frame); the released control point (frames 3, 4)
    # is the reference's value on every rank -- Dx of the last project() (AnchorForce.cpp:80-83), i.e. the node BEFORE the last
    # global solve: the owner rank's state travels through admm_hip_allreduce_host
    (X1, cp1), (Xw, cpw) = run(5, 10, "b")
    assert np.abs(Xw - X1).max() < 2e-5
    assert np.abs(cpw - cp1).max() < 2e-5
    assert 0.0 < np.abs(cp1 - X1[-1][3 * moving:3 * moving + 3]).max() < 1e-2      # (not the node after the frame)


@pytest.mark.gpu
def test_plinko_scene_through_class_api(pkg, tmp_path):
    g = golden("traj_collision.npz")
    n = g["x"].shape[0]
    inp = tmp_path / "in.bin"; outp = tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("3i", n, g["tets"].shape[0], g["types"].size))
        f.write(g["x"].astype(np.float64).tobytes()); f.write(np.repeat(g["mass"], 3).tobytes()); f.write(g["tets"].astype(np.int32).tobytes())
        f.write(g["types"].astype(np.int32).tobytes()); f.write(g["params"].astype(np.float64).tobytes())
    frames = int(g["frames"][-1]) + 1
    r = subprocess.run([compile_cpp("scene_plinko", pkg), str(inp), str(outp), str(frames), str(int(g["iters"]))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "weight 32" in r.stdout and "global_idx %d" % (9 * g["tets"].shape[0]) in r.stdout
    X = np.fromfile(outp, dtype=np.float64).reshape(frames, 3 * n)
    for fi, f in enumerate(g["frames"]):
        assert np.abs(X[f] - g["x_frames"][fi]).max() < 1e-9      # the compiled reference's trajectory


# ---------------------------------------------------------------------------------------------------------------
# "existing ForceBuilder + SimContext scenes drop in unchanged" and the plug-in surface (b)
# ---------------------------------------------------------------------------------------------------------------
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
DILLO_XML = os.path.join(ROOT, "tests", "golden", "scenes", "poordillo", "poordillo.xml")


def test_reference_callers_compile_and_link_unchanged(pkg):
    """Build container only: the reference's OWN samples/singletet.cpp, samples/singlenode.cpp, src/SimContext.cpp and
    src/ForceBuilder.cpp, untouched and from where they lie, compile and LINK against the class mirror host/admm (through
    the per-class forwarding headers they include) and libadmm_hip.so (oracle/Makefile hip_callers).  Without a GPU the
    resulting programs get as far as System::initialize() and fail loudly there."""
    if not os.path.isdir("/root/reference/src"):
        pytest.skip("the reference tree is only present in the build container")
    pkg.lib()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "hip_callers"])
    for exe in ("singletet_hip", "singlenode_hip", "dillo_hip"):
        assert os.path.exists(os.path.join(REF_BIN, exe))
    if have_gpu():
        return
    r = subprocess.run([os.path.join(REF_BIN, "singletet_hip")], capture_output=True, text=True)
    assert "no usable HIP device" in r.stderr          # singletet.cpp:37 returns 0 when initialize() fails
    r = subprocess.run([os.path.join(REF_BIN, "dillo_hip"), DILLO_XML, os.devnull, "1"], capture_output=True, text=True)
    assert r.returncode != 0 and "Tetmesh dillo has 2761 tets" in r.stdout and "no usable HIP device" in r.stderr


def _run_user_force(pkg, tmp_path, mode, g):
    out = tmp_path / ("uf%d.bin" % mode)
    r = subprocess.run([compile_cpp("user_force", pkg), str(mode), str(out), str(int(g["frames"])), str(int(g["iters"])), str(int(g["n"]))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = np.fromfile(out, dtype=np.float64)
    n3 = 3 * int(g["n"]) ** 2
    nf = int(g["frames"])
    return raw[:nf * n3].reshape(nf, n3), raw[nf * n3:].reshape(-1, 2)


@pytest.mark.gpu
def test_user_spring_matches_builtin_bit_for_bit(pkg, tmp_path):
    """A user-written admm::Force subclass doing Spring's arithmetic (tests/cpp/user_force.cpp MySpring; its project() runs
    on the host, Dx and the right-hand side on the device) against the built-in ADMM_KIND_SPRING kernel: every frame of the
    trajectory is bitwise the same.  (The real reference agrees with itself the same way: make_golden_user.py asserts it.)"""
    g = golden("user_force.npz")
    x0, _ = _run_user_force(pkg, tmp_path, 0, g)
    x1, gw = _run_user_force(pkg, tmp_path, 1, g)
    assert np.array_equal(x0, x1)
    assert np.array_equal(gw, g["gw_mode1"])            # global_idx = 0, 3, 6, ... and weight = sqrt(k), as in the reference
    assert np.abs(x1 - g["x_mode1"]).max() < 1e-9        # and the compiled reference's trajectory (different elimination order)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 3])
def test_user_plugins_vs_compiled_reference(pkg, tmp_path, mode):
    """User-written Force (ShellForce), ExplicitForce (SwirlForce) and CollisionShape (SlabShape, which turns its
    CollisionForce into a host-projected force) -- the same source file compiled with the real reference produced the
    fixture (tests/golden/make_golden_user.py)."""
    g = golden("user_force.npz")
    x, gw = _run_user_force(pkg, tmp_path, mode, g)
    assert np.abs(x - g["x_mode%d" % mode]).max() < 1e-8
    assert np.array_equal(gw[:, 1], g["gw_mode%d" % mode][:, 1])        # weights


def _check_dillo(out, g, release):
    hdr = np.fromfile(out, dtype=np.int32, count=3)
    assert hdr[0] == int(g["dof"]) and hdr[1] == int(g["n_hand"]) and hdr[2] == int(g["n_foot"])     # same grabbed vertices
    raw = np.fromfile(out, dtype=np.float64, offset=12)
    nf = int(g["frames"]); dof = int(g["dof"])
    X = raw[:nf * dof].reshape(nf, dof)
    assert np.isfinite(X).all()
    if release < 0:
        ref, env, frames = g["x_frames"], g["ulp_sensitivity"], range(nf)
    else:
        ref, env, frames = g["x_release"], g["ulp_sensitivity_release"], [int(f) for f in g["release_keep"]]
    # The reference's own resolution: its trajectory moves by `env` when its start moves by 1-3 ulps (truncated L-BFGS +
    # Armadillo contacts).  Two separate claims:
    #  (1) PRE-CHAOS frames (the reference still agrees with itself to < 1e-4; frames 0-2 here): a tight bound, 3 x the reference's
    #      own sensitivity (measured: 0.5-1.2 x) -- a regression of the solver shows up HERE and cannot hide behind (2);
    #  (2) frames after the reference's own bifurcation (its 1-ulp twin is 5e-3 .. 3e-2 away): these assert the same macroscopic
    #      motion inside 5 x that chaotic envelope (measured: 0.3-1.5 x) and finiteness -- no more can be asked of ANY solver
    #      whose rounding differs from the reference's.
    tight = [(k, f) for k, f in enumerate(frames) if float(env[k]) < 1e-4]
    assert release >= 0 or len(tight) >= 3
    for k, f in tight:
        err = np.abs(X[f] - ref[k]).max()
        assert err < 3.0 * float(env[k]), ("pre-chaos frame", f, err, float(env[k]))
    for k, f in enumerate(frames):
        e = float(env[k])
        err = np.abs(X[f] - ref[k]).max()
        if os.environ.get("ADMM_TEST_VERBOSE"):
            print("dillo frame %3d: |x - x_ref| %.3e   reference's own 1-3 ulp sensitivity %.3e" % (f, err, e))
        if e >= 1e-4:
            assert err < 5.0 * e, ("chaotic frame", f, err, e)
    if release >= 0:
        assert np.abs(raw[nf * dof:] - g["hand_cp_after_release"]).max() < 5.0 * float(env[-1])      # a released anchor follows its node
    else:
        assert np.abs(X[-1] - X[0]).max() > 1.9              # the grabbers really dragged hand and foot 2 m apart


@pytest.mark.gpu
@pytest.mark.parametrize("release", [-1, 30])
def test_poordillo_scripted_grabbers(pkg, tmp_path, release):
    """BASELINE.json configs[2] as SURVEY 8(d) config 3 specifies it: the shipped armadillo with the sample's MovingAnchors
    on hand and foot dragged by smooth_move over t in [1, 3] s (and, second case, the hand released at frame 30 through
    weight = 0 + recompute_weights), loaded from the XML by the headless SimContext, against the compiled reference's
    trajectory within the reference's own 1-3 ulp sensitivity envelope, frame by frame."""
    g = golden("traj_dillo_grab.npz")
    out = tmp_path / "d.bin"
    r = subprocess.run([compile_cpp("dillo_main", pkg), DILLO_XML, str(out), str(int(g["frames"])), str(release)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    _check_dillo(out, g, release)


@pytest.mark.gpu
def test_reference_programs_run_on_the_gpu(pkg, tmp_path):
    """The binaries of test_reference_callers_compile_and_link_unchanged travel with the snapshot (oracle/_ref/): the
    reference's own sample mains and scene layer, running on the MI355X through the mirror.  singletet prints the
    reference's known answer; the poordillo script through the REFERENCE's SimContext/ForceBuilder matches the fixture."""
    if not os.path.exists(os.path.join(REF_BIN, "singletet_hip")):
        pytest.skip("oracle/_ref/*_hip not built (they need the reference tree)")
    pkg.lib()
    r = subprocess.run([os.path.join(REF_BIN, "singletet_hip")], capture_output=True, text=True)
    assert r.returncode == 0 and "Node 4 x: 171.571" in r.stdout, r.stdout + r.stderr
    # the same UNCHANGED binary under a launcher's environment: ADMM_HIP_RANKS_FROM_ENV=1 makes System::initialize() take rank / world / GPU
    # from it (a one-rank launch here: the multi-rank form needs one GPU per rank for RCCL) -- same answer; a rank outside the world is refused
    env = dict(os.environ, ADMM_HIP_RANKS_FROM_ENV="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([os.path.join(REF_BIN, "singletet_hip")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "Node 4 x: 171.571" in r.stdout, r.stdout + r.stderr
    env = dict(os.environ, ADMM_HIP_RANKS_FROM_ENV="1", RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", MASTER_PORT="29777", ADMM_HIP_RCCL_ID_FILE=str(tmp_path / "id"))
    env.pop("ADMM_HIP_RCCL_LIB", None)
    r = subprocess.run([os.path.join(REF_BIN, "singletet_hip")], capture_output=True, text=True, env=dict(env, RANK="5"), timeout=120)
    assert "171.571" not in r.stdout and "shard.rank 5 outside [0, 2)" in r.stderr, r.stdout + r.stderr
    r = subprocess.run([os.path.join(REF_BIN, "singlenode_hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for want in ("-9.8", "-29.4", "-58.8", "-98"):
        assert want in r.stdout
    g = golden("traj_dillo_grab.npz")
    out = tmp_path / "d.bin"
    r = subprocess.run([os.path.join(REF_BIN, "dillo_hip"), DILLO_XML, str(out), str(int(g["frames"])), "-1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    _check_dillo(out, g, -1)
