"""ctypes bindings of the two TEST-ONLY checkers:

  * ``Oracle``  -- oracle/liboracle.so, our C restatement of the reference path
  * ``Ref``     -- oracle/_ref/libadmm_ref.so, the REAL reference compiled from
                   /root/reference (only exists where oracle/Makefile built it)

Nothing in the product package imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")

KIND = dict(ANCHOR=0, SPRING=1, TET_LINEAR=2, TET_VOLUME=3, TET_NH=4, TET_STVK=5, TRI_STRAIN=6, BEND=7, COLLISION=8, TRI_AREA=9, TRI_FUNG=10)
KIND_NODES = [1, 2, 4, 4, 4, 4, 3, 4, 1, 3, 3]
KIND_ROWS = [3, 3, 9, 9, 9, 9, 6, 9, 3, 6, 6]
KIND_PARAMS = [2, 1, 1, 3, 3, 3, 4, 1, 1, 4, 3]

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)


def _d(a):
    return a.ctypes.data_as(dp)


def _i(a):
    return a.ctypes.data_as(ip)


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "liboracle.so"])
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "ref"])


def have_ref():
    """The compiled reference (oracle/_ref, built from /root/reference where that exists -- this container; the GPU box
    only has what was built here).  Built on first use so that the suite does not depend on __graft_entry__.build() having run."""
    lib = os.path.join(ORACLE_DIR, "_ref", "libadmm_ref.so")
    if not os.path.exists(lib) and os.path.isdir("/root/reference"):
        subprocess.call(["make", "-s", "-C", ORACLE_DIR, "ref"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(lib)


def deformed_start(x0):
    """A smooth, LARGE deformation of a bar's rest positions built from + and * only (no transcendental, no division: the same
    bits on every host and every numpy build): shear, bending and twist-like terms that put the deformation gradients 5-20 %
    away from the identity.  The start of the one-iteration full-size fixture (tests/golden/traj_bar_1M_one_iter.npz): with it
    the single local step of that frame is a real Neo-Hookean prox for every tet instead of the identity."""
    p = np.asarray(x0, dtype=np.float64).reshape(-1, 3)
    q = p.copy()
    q[:, 0] = p[:, 0] + 0.02 * (p[:, 1] * p[:, 2])
    q[:, 1] = p[:, 1] - 0.004 * (p[:, 2] * p[:, 2])
    q[:, 2] = p[:, 2] + 0.03 * (p[:, 0] * p[:, 1])
    return q.ravel()


def solve_rhs(seed, x0, m3):
    """The three right-hand sides of the direct solve fixtures (tests/golden/solve_*.npz; 3n doubles each, node-major like
    System::m_x): white noise, an M x_bar-like smooth vector (mass x displaced positions, what System.cpp:61 feeds the solver),
    and one unit spike (a column of A^-1)."""
    rng = np.random.default_rng(int(seed))
    x0 = np.asarray(x0, dtype=np.float64).ravel(); m3 = np.asarray(m3, dtype=np.float64).ravel()
    n = x0.size
    b0 = rng.normal(size=n)
    b1 = m3 * (x0 + 0.01 * np.sin(7.0 * x0 + 0.3 * np.arange(n)))
    b2 = np.zeros(n); b2[int(rng.integers(0, n))] = 1.0
    return np.stack([b0, b1, b2])


class _Sys:
    """Common python face of oracle / reference systems."""

    prefix = None
    lib = None

    def _f(self, name):
        return getattr(self.lib, self.prefix + name)

    def settings(self, dt, iters):
        raise NotImplementedError

    def add_nodes(self, x, m):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        m = np.ascontiguousarray(m, dtype=np.float64).ravel()
        self.m3 = np.concatenate([getattr(self, "m3", np.zeros(0)), m])      # the masses this system was given (RhsReference)
        return self._f("add_nodes")(self.h, x.size, _d(x), _d(m))

    def add_forces(self, kind, idx, params):
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, KIND_NODES[kind])
        n = idx.shape[0]
        params = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64), (n, KIND_PARAMS[kind])))
        r = self._f("add_forces")(self.h, kind, n, _i(idx), _d(params))
        assert r >= 0
        return r

    def add_moving_anchor(self, idx, pos, active=True, weight=-1.0):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        return self._f("add_moving_anchor")(self.h, int(idx), _d(pos), int(active), float(weight))

    def set_control_point(self, handle, pos, active=True):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        self._f("set_control_point")(self.h, handle, _d(pos), int(active))

    def add_gravity(self, g):
        self._f("add_gravity")(self.h, float(g[0]), float(g[1]), float(g[2]))

    def initialize(self):
        return bool(self._f("initialize")(self.h))

    def step(self):
        return bool(self._f("step")(self.h))

    @property
    def dof(self):
        return self._f("dof")(self.h)

    @property
    def rows(self):
        return self._f("rows")(self.h)

    @property
    def n_forces(self):
        return self._f("n_forces")(self.h)

    def D_triplets(self):
        n = self._f("D_nnz")(self.h)
        r = np.zeros(n, np.int32); c = np.zeros(n, np.int32); v = np.zeros(n)
        self._f("get_D")(self.h, _i(r), _i(c), _d(v))
        return r, c, v

    def L_nnz(self):
        return self._f("L_nnz")(self.h)

    def time_steps(self, frames):
        return self._f("time_steps")(self.h, frames)


class Ref(_Sys):
    prefix = "ref_"

    @classmethod
    def load(cls):
        if cls.lib is None:
            lib = C.CDLL(os.path.join(ORACLE_DIR, "_ref", "libadmm_ref.so"))
            lib.ref_create.restype = C.c_void_p
            for n in ("destroy", "settings", "set_control_point", "add_gravity", "get_x", "set_x", "get_v", "set_v", "get_u",
                      "get_z", "get_wdiag", "get_D", "svd3", "svd32", "recompute_weights", "set_force_weight", "get_masses",
                      "get_control_point", "add_wind"):
                getattr(lib, "ref_" + n).restype = None
            lib.ref_D_nnz.restype = C.c_long
            lib.ref_L_nnz.restype = C.c_long
            lib.ref_force_weight.restype = C.c_double
            lib.ref_time_steps.restype = C.c_double
            lib.ref_elapsed.restype = C.c_double
            lib.ref_settings.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
            lib.ref_add_gravity.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
            lib.ref_add_moving_anchor.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, C.c_double]
            lib.ref_set_force_weight.argtypes = [C.c_void_p, C.c_int, C.c_double]
            lib.ref_add_wind.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, C.c_double]
            lib.ref_add_explicit_subset.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, C.c_double]
            lib.ref_add_explicit_subset.restype = None
            lib.ref_set_explicit_dir.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
            lib.ref_set_explicit_dir.restype = None
            lib.ref_add_collision.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double]
            lib.ref_project_single.argtypes = [C.c_int, dp, dp, C.c_double, C.c_int, dp, dp, dp, dp, dp, ip, dp]
            for n in ("add_nodes", "add_forces", "set_control_point", "initialize", "step", "dof", "rows", "n_forces",
                      "get_x", "set_x", "get_v", "set_v", "get_u", "get_z", "get_wdiag", "force_global_idx", "force_weight",
                      "D_nnz", "get_D", "L_nnz", "get_hyper_state", "set_hyper_state", "time_steps", "destroy",
                      "recompute_weights", "get_masses", "get_control_point", "elapsed"):
                fn = getattr(lib, "ref_" + n)
                if fn.argtypes is None:
                    fn.argtypes = None  # first arg is the handle; set below where needed
            cls.lib = lib
        return cls.lib

    def __init__(self):
        self.load()
        self.h = C.c_void_p(self.lib.ref_create())

    def __del__(self):
        try:
            self.lib.ref_destroy(self.h)
        except Exception:
            pass

    def settings(self, dt, iters):
        self.lib.ref_settings(self.h, dt, iters, 0)

    def _vec(self, name, n):
        a = np.zeros(n)
        getattr(self.lib, "ref_get_" + name)(self.h, _d(a))
        return a

    @property
    def x(self):
        return self._vec("x", self.dof)

    @x.setter
    def x(self, val):
        val = np.ascontiguousarray(val, dtype=np.float64)
        self.lib.ref_set_x(self.h, _d(val))

    @property
    def v(self):
        return self._vec("v", self.dof)

    @property
    def masses(self):
        return self._vec("masses", self.dof)

    @property
    def u(self):
        return self._vec("u", self.rows)

    @property
    def z(self):
        return self._vec("z", self.rows)

    @property
    def wdiag(self):
        return self._vec("wdiag", self.rows)

    def global_idx(self):
        return np.array([self.lib.ref_force_global_idx(self.h, i) for i in range(self.n_forces)], np.int64)

    def weights(self):
        return np.array([self.lib.ref_force_weight(self.h, i) for i in range(self.n_forces)])

    def hyper_state(self, i):
        st = np.zeros(4)
        it = self.lib.ref_get_hyper_state(self.h, i, _d(st))
        return st, it

    def add_wind(self, tris, direction):
        tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        self.lib.ref_add_wind(self.h, tris.shape[0], _i(tris), *[float(d) for d in direction])

    def add_explicit_subset(self, idx, g):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.lib.ref_add_explicit_subset(self.h, idx.size, _i(idx), float(g[0]), float(g[1]), float(g[2]))

    def set_explicit_dir(self, which, g):
        self.lib.ref_set_explicit_dir(self.h, which, float(g[0]), float(g[1]), float(g[2]))

    def add_collision(self, types, params, weight=32.0):
        t = np.ascontiguousarray(types, dtype=np.int32); p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 4)
        return self.lib.ref_add_collision(self.h, t.size, _i(t), _d(p), float(weight))

    def recompute_weights(self):
        self.lib.ref_recompute_weights(self.h)

    def set_force_weight(self, i, w):
        self.lib.ref_set_force_weight(self.h, i, w)

    def solve(self, b):
        """x = solver.solve(b) on the reference's own SimplicialLDLT of the 3n x 3n system (System.cpp:62,
        SimplicialCholesky.h:153-177) -- reached through the derived-class accessor of oracle/ref_shim.cpp"""
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        assert b.size == self.dof
        x = np.zeros_like(b)
        self.lib.ref_solve(self.h, _d(b), _d(x))
        return x

    @classmethod
    def project_single(cls, kind, x_rest, params, Dx, u0=None, state=None, dt=0.04):
        """n_calls consecutive project() calls of one stand-alone element."""
        lib = cls.load()
        rows = KIND_ROWS[kind]
        Dx = np.ascontiguousarray(Dx, dtype=np.float64).reshape(-1, rows)
        n = Dx.shape[0]
        u = np.zeros(rows) if u0 is None else np.array(u0, dtype=np.float64)
        z_out = np.zeros((n, rows)); u_out = np.zeros((n, rows))
        st = np.array([1, 1, 1, 1], dtype=np.float64) if state is None else np.array(state, dtype=np.float64)
        iters = np.zeros(n, np.int32)
        init = np.zeros(16)
        x_rest = np.ascontiguousarray(x_rest, dtype=np.float64)
        params = np.ascontiguousarray(params, dtype=np.float64)
        r = lib.ref_project_single(kind, _d(x_rest), _d(params), dt, n, _d(Dx), _d(u), _d(z_out), _d(u_out), _d(st), _i(iters), _d(init))
        assert r == 0
        return dict(z=z_out, u=u_out, state=st, n_iters=iters, init=init)

    @classmethod
    def svd3(cls, F):
        lib = cls.load()
        F = np.ascontiguousarray(F, dtype=np.float64)
        U = np.zeros(9); S = np.zeros(3); V = np.zeros(9)
        lib.ref_svd3(_d(F), _d(U), _d(S), _d(V))
        return U, S, V

    @classmethod
    def svd32(cls, F):
        lib = cls.load()
        F = np.ascontiguousarray(F, dtype=np.float64)
        U = np.zeros(9); S = np.zeros(2); V = np.zeros(4)
        lib.ref_svd32(_d(F), _d(U), _d(S), _d(V))
        return U, S, V


class OrcForce(C.Structure):
    _fields_ = [("kind", C.c_int), ("idx", C.c_int * 4), ("params", C.c_double * 4), ("weight", C.c_double),
                ("B", C.c_double * 12), ("measure", C.c_double), ("alpha", C.c_double * 4), ("pos", C.c_double * 3),
                ("active", C.c_int), ("moving", C.c_int), ("state", C.c_double * 4), ("n_iters", C.c_int),
                ("n_fev", C.c_int), ("global_idx", C.c_int)]


class Oracle(_Sys):
    prefix = "orc_"

    @classmethod
    def load(cls):
        if cls.lib is None:
            path = os.path.join(ORACLE_DIR, "liboracle.so")
            if not os.path.exists(path):
                build_oracle()
            lib = C.CDLL(path)
            lib.orc_create.restype = C.c_void_p
            for n in ("x", "v", "u", "z", "wdiag"):
                getattr(lib, "orc_" + n).restype = dp
                getattr(lib, "orc_" + n).argtypes = [C.c_void_p]
            lib.orc_get_force.restype = C.POINTER(OrcForce)
            lib.orc_get_force.argtypes = [C.c_void_p, C.c_int]
            lib.orc_D_nnz.restype = C.c_long
            lib.orc_L_nnz.restype = C.c_long
            lib.orc_time_steps.restype = C.c_double
            lib.orc_settings.argtypes = [C.c_void_p, C.c_double, C.c_int]
            lib.orc_set_layout.argtypes = [C.c_void_p, C.c_int]
            lib.orc_add_gravity.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
            lib.orc_add_moving_anchor.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, C.c_double]
            lib.orc_force_construct.argtypes = [C.POINTER(OrcForce), C.c_int, ip, dp]
            lib.orc_force_initialize.argtypes = [C.POINTER(OrcForce), dp]
            lib.orc_force_project.argtypes = [C.POINTER(OrcForce), C.c_double, dp, dp, dp]
            lib.orc_add_explicit.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, ip]
            lib.orc_set_collision_shapes.argtypes = [C.c_void_p, C.c_int, ip, dp]
            lib.orc_track_residuals.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
            lib.orc_track_residuals.restype = None
            lib.orc_get_residuals.argtypes = [C.c_void_p, dp, dp, C.c_int]
            lib.orc_recompute_weights.argtypes = [C.c_void_p]
            for n in ("settings", "set_layout", "add_gravity", "destroy", "get_D", "set_control_point", "svd3", "svd32", "add_explicit", "set_collision_shapes",
                      "oriented_svd", "force_construct", "force_initialize", "force_project"):
                getattr(lib, "orc_" + n).restype = None
            cls.lib = lib
        return cls.lib

    def __init__(self, ref_layout=False):
        self.load()
        self.h = C.c_void_p(self.lib.orc_create())
        self.lib.orc_set_layout(self.h, int(ref_layout))

    def __del__(self):
        try:
            self.lib.orc_destroy(self.h)
        except Exception:
            pass

    def settings(self, dt, iters):
        self.lib.orc_settings(self.h, dt, iters)

    def track_residuals(self, on=True, tol_r=0.0, tol_s=0.0):
        self.lib.orc_track_residuals(self.h, int(on), float(tol_r), float(tol_s))

    def residuals(self):
        r = np.zeros(256); s = np.zeros(256)
        n = self.lib.orc_get_residuals(self.h, _d(r), _d(s), 256)
        return r[:n], s[:n], n

    def _view(self, name, n):
        p = getattr(self.lib, "orc_" + name)(self.h)
        return np.ctypeslib.as_array(p, shape=(n,)) if n else np.zeros(0)

    @property
    def x(self):
        return self._view("x", self.dof).copy()

    @x.setter
    def x(self, val):
        self._view("x", self.dof)[:] = val

    @property
    def v(self):
        return self._view("v", self.dof).copy()

    @property
    def u(self):
        return self._view("u", self.rows).copy()

    @property
    def z(self):
        return self._view("z", self.rows).copy()

    @property
    def wdiag(self):
        return self._view("wdiag", self.rows).copy()

    def add_explicit(self, type_, direction, idx=None):
        d = np.ascontiguousarray(direction, dtype=np.float64)
        ix = np.zeros(0, np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        n = ix.size // 3 if type_ == 1 else ix.size
        self.lib.orc_add_explicit(self.h, type_, _d(d), n, _i(ix))

    def set_collision_shapes(self, types, params):
        t = np.ascontiguousarray(types, dtype=np.int32); p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 4)
        self.lib.orc_set_collision_shapes(self.h, t.size, _i(t), _d(p))

    def force(self, i):
        return self.lib.orc_get_force(self.h, i).contents

    def global_idx(self):
        return np.array([self.force(i).global_idx for i in range(self.n_forces)], np.int64)

    def weights(self):
        return np.array([self.force(i).weight for i in range(self.n_forces)])

    def hyper_state(self, i):
        f = self.force(i)
        return np.array(list(f.state)), f.n_iters

    def set_weights(self, w):
        """every force's weight member (Force::weight), then System::recompute_weights"""
        for i, wi in enumerate(np.asarray(w, dtype=np.float64)):
            self.force(i).weight = float(wi)
        assert self.lib.orc_recompute_weights(self.h) == 1

    def solve(self, b):
        """the oracle's LDL^T solve of the same 3n x 3n system (admm_oracle.c ldl_solve = SimplicialCholesky.h:153-177)"""
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        assert b.size == self.dof
        x = np.zeros_like(b)
        self.lib.orc_solve(self.h, _d(b), _d(x))
        return x

    def local_step(self, xcur, dt=0.04):
        """ONE local step of the oracle on caller-supplied positions: Dx = D x_cur accumulated column-ascending like Eigen's
        column-major product (System.cpp:54), then project() of every force in list order (System.cpp:57-58) on the oracle's
        own u and warm-start state.  Returns flat (u, z) in the oracle's (compact) row layout; per force: rows
        global_idx .. global_idx + KIND_ROWS[kind]."""
        rr, cc, vv = self.D_triplets()
        Dx = np.zeros(self.rows)
        k = np.lexsort((cc, rr))
        for r_, c_, v_ in zip(rr[k], cc[k], vv[k]):
            Dx[r_] += v_ * xcur[c_]
        u = self._view("u", self.rows); z = self._view("z", self.rows)
        for i in range(self.n_forces):
            f = self.lib.orc_get_force(self.h, i)
            g = f.contents.global_idx; rows = KIND_ROWS[f.contents.kind]
            d = np.ascontiguousarray(Dx[g:g + rows]); uu = np.ascontiguousarray(u[g:g + rows]); zz = np.zeros(rows)
            self.lib.orc_force_project(f, float(dt), _d(d), _d(uu), _d(zz))
            u[g:g + rows] = uu; z[g:g + rows] = zz
        return u.copy(), z.copy()

    @classmethod
    def project_single(cls, kind, x_rest, params, Dx, u0=None, state=None, dt=0.04):
        lib = cls.load()
        rows = KIND_ROWS[kind]
        Dx = np.ascontiguousarray(Dx, dtype=np.float64).reshape(-1, rows)
        n = Dx.shape[0]
        f = OrcForce()
        idx = np.arange(4, dtype=np.int32)
        params = np.ascontiguousarray(params, dtype=np.float64)
        x_rest = np.ascontiguousarray(x_rest, dtype=np.float64)
        lib.orc_force_construct(C.byref(f), kind, _i(idx), _d(params))
        lib.orc_force_initialize(C.byref(f), _d(x_rest))
        if state is not None:
            for j in range(4):
                f.state[j] = state[j]
        u = np.zeros(rows) if u0 is None else np.array(u0, dtype=np.float64)
        z = np.zeros(rows)
        z_out = np.zeros((n, rows)); u_out = np.zeros((n, rows)); iters = np.zeros(n, np.int32); fev = np.zeros(n, np.int32)
        for c in range(n):
            d = np.ascontiguousarray(Dx[c])
            lib.orc_force_project(C.byref(f), dt, _d(d), _d(u), _d(z))
            z_out[c] = z; u_out[c] = u; iters[c] = f.n_iters; fev[c] = f.n_fev
        init = np.zeros(16)
        init[0] = f.weight
        if kind in (2, 3, 4, 5):
            init[1:13] = list(f.B); init[13] = f.measure
        elif kind in (6, 9, 10):
            init[1:7] = list(f.B)[:6]; init[7] = f.measure
        elif kind == 7:
            init[1:5] = list(f.alpha)
        elif kind == 1:
            init[1] = f.measure
        return dict(z=z_out, u=u_out, state=np.array(list(f.state)), n_iters=iters, n_fev=fev, init=init)

    @classmethod
    def svd3(cls, F):
        lib = cls.load()
        F = np.ascontiguousarray(F, dtype=np.float64)
        U = np.zeros(9); S = np.zeros(3); V = np.zeros(9)
        lib.orc_svd3(_d(F), _d(U), _d(S), _d(V))
        return U, S, V

    @classmethod
    def svd32(cls, F):
        lib = cls.load()
        F = np.ascontiguousarray(F, dtype=np.float64)
        U = np.zeros(9); S = np.zeros(2); V = np.zeros(4)
        lib.orc_svd32(_d(F), _d(U), _d(S), _d(V))
        return U, S, V


def extreme_matrices(rng, n):
    """3x3 inputs (row-major 9-vectors of D_i x in the device's row order) that walk the corners of the Jacobi SVD and the proxes: every
    power-of-ten scale the format holds, entries 300 decades apart inside one matrix, rank 0 / 1 / 2, diagonal, permutation, symmetric
    and antisymmetric 2x2 blocks (the t == 0 branch of real_2x2_jacobi_svd), off-diagonals at the rotation threshold, repeated
    singular values, inverted and reflected matrices, infinities and NaNs."""
    M = []
    base = rng.normal(size=(n, 3, 3))
    for k, e in enumerate([-305, -300, -200, -160, -154, -150, -100, -20, -8, 0, 8, 20, 100, 150, 154, 160, 200, 300, 305]):
        M.append(base[k] * 10.0 ** e)
    for k in range(40):                       # rows / columns / entries scaled by wildly different powers of ten
        A = rng.normal(size=(3, 3))
        if k % 3 == 0: A = A * 10.0 ** rng.uniform(-300, 0, size=(3, 1))
        elif k % 3 == 1: A = A * 10.0 ** rng.uniform(-300, 0, size=(1, 3))
        else: A = A * 10.0 ** rng.uniform(-160, 0, size=(3, 3))
        M.append(A)
    I = np.eye(3)
    M += [np.zeros((3, 3)), I, -I, 2.5 * I, I[[1, 2, 0]], I[[2, 1, 0]], np.diag([3.0, 2.0, 1.0]), np.diag([1.0, 1.0, 1e-300]), np.diag([1e-200, 1.0, 1e200]),
          np.diag([1.0, -1.0, 1.0]), np.diag([-2.0, -3.0, -4.0])]
    for k in range(10):                        # rank one and rank two
        a, b = rng.normal(size=3), rng.normal(size=3)
        M.append(np.outer(a, b)); M.append(np.outer(a, b) + np.outer(rng.normal(size=3), rng.normal(size=3)))
    for eps in (0.0, 1e-17, 2.2e-16, 4.5e-16, 1e-15, 1e-8, 1e-3):     # a 2x2 block at the rotation threshold, symmetric / antisymmetric / one-sided
        for sym in (1.0, -1.0, 0.0):
            A = np.diag([1.0, 1.0 + 1e-9, 0.5]); A[0, 1] = eps; A[1, 0] = sym * eps; M.append(A)
            A = np.diag([1.0, -1.0, 0.5]); A[0, 1] = eps; A[1, 0] = sym * eps; M.append(A)      # t = m00 + m11 == 0
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]])
    M += [R, R @ np.diag([2.0, 2.0, 1.0]), R @ np.diag([1.0, 1.0, 1.0]) @ R.T, -R]
    for v in (np.inf, -np.inf, np.nan):
        A = rng.normal(size=(3, 3)); A[1, 2] = v; M.append(A)
    while len(M) < n:
        M.append(rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-3, 4))
    return np.array(M[:n]).reshape(n, 9)


def edge_rows(Dx, rows):
    """Dx [n][rows] (extreme_matrices cut to a kind's row count) with the rows the closed-form kinds branch on made sure of: all zero
    (Spring's nrm <= 0), all denormal, around 1e+160 and 1e-160 (the squares of a norm overflow / underflow), one and all entries
    infinite, one and all NaN -- written over the tail (the generic fill) where missing.  -> (Dx, dict name -> row index of one)."""
    Dx = np.array(Dx[:, :rows], dtype=np.float64)
    a = np.abs(Dx)
    fin = np.isfinite(Dx).all(axis=1)
    tests = dict(zero=lambda: (Dx == 0).all(axis=1),
                 denormal=lambda: ((a > 0) & (a < np.finfo(np.float64).tiny)).all(axis=1),
                 huge=lambda: fin & (a.max(axis=1) > 1e155) & (a.max(axis=1) < 1e165),
                 tiny=lambda: (a.max(axis=1) < 1e-155) & (a.max(axis=1) > 1e-165),
                 inf=lambda: np.isinf(Dx).any(axis=1) & ~np.isnan(Dx).any(axis=1),
                 all_inf=lambda: np.isinf(Dx).all(axis=1),
                 nan=lambda: np.isnan(Dx).any(axis=1),
                 all_nan=lambda: np.isnan(Dx).all(axis=1))
    ramp = 1.0 + 0.25 * np.arange(rows)
    fill = dict(zero=0.0 * ramp, denormal=3e-310 * ramp, huge=-1.1e160 * ramp, tiny=1.3e-160 * ramp, inf=np.where(np.arange(rows) == 1, np.inf, ramp),
                all_inf=np.where(np.arange(rows) % 2 == 0, np.inf, -np.inf), nan=np.where(np.arange(rows) == rows - 1, np.nan, ramp), all_nan=np.nan * ramp)
    where, tail = {}, Dx.shape[0] - 1
    for name, test in tests.items():
        hit = np.flatnonzero(test())
        if hit.size == 0:
            Dx[tail] = fill[name]; a = np.abs(Dx); fin = np.isfinite(Dx).all(axis=1)
            hit = np.array([tail]); tail -= 1
        where[name] = int(hit[0])
    for name, test in tests.items():      # (a later fill never lands on an earlier find: the tail is generic rows only)
        assert test()[where[name]], name
    return Dx, where


HYPER_CAPS, HYPER_CAPS_WIDE = (1, 3, 5), (1, 3, 5, 7, 10, 12)


def het_params(kind, n, rng, caps=HYPER_CAPS):
    """[n][KIND_PARAMS[kind]] constructor parameters that differ from element to element, drawn (never sorted: nothing follows the
    element order): stiffness-like entries log-uniform over 2.5 decades (mu, lambda: four); TET_VOLUME limits in [0.7, 1] / [1, 1.3]; TRI_STRAIN limits in
    [0.8, 1] / [1, 1.2] and the strain-limiting flag from {0, 1}; TRI_AREA 1..6 iterations; TRI_FUNG mu in [5, 500] with the limits of
    test_local_step_fung; about 30 % of the ANCHORs with use_weight <= 0 (-1 or 0: the 1000.f default); the hyperelastic kinds'
    max_iterations from `caps`."""
    name = {v: k for k, v in KIND.items()}[kind]
    stiff = lambda lo, hi: 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), size=n)      # noqa: E731
    if name == "ANCHOR":
        w = stiff(10.0, 3000.0)
        off = rng.random(n) < 0.3
        w[off] = rng.choice([-1.0, 0.0], size=int(off.sum()))
        cols = [w, np.ones(n)]
    elif name in ("SPRING", "TET_LINEAR", "BEND", "COLLISION"):
        cols = [stiff(3.0, 1000.0)]
    elif name == "TET_VOLUME":
        cols = [stiff(3.0, 1000.0), rng.uniform(0.7, 1.0, size=n), rng.uniform(1.0, 1.3, size=n)]
    elif name in ("TET_NH", "TET_STVK"):
        # four decades, mu and lambda drawn apart: the L-BFGS count grows with lambda / mu and with the stiffness itself (its gradient
        # tolerance is absolute), and the caps of 10 and 12 only bind on the slow tail (test_batch_parameters.cap_condition)
        cols = [stiff(1e2, 1e6), stiff(1e2, 1e6), rng.choice(np.asarray(caps, dtype=np.float64), size=n)]
    elif name == "TRI_STRAIN":
        cols = [stiff(3.0, 1000.0), rng.uniform(0.8, 1.0, size=n), rng.uniform(1.0, 1.2, size=n), rng.integers(0, 2, size=n).astype(np.float64)]
    elif name == "TRI_AREA":
        cols = [stiff(3.0, 1000.0), rng.integers(1, 7, size=n).astype(np.float64), rng.uniform(0.8, 1.0, size=n), rng.uniform(1.0, 1.2, size=n)]
    elif name == "TRI_FUNG":
        cols = [stiff(5.0, 500.0), np.full(n, 0.5), np.full(n, 2.0)]
    else:
        raise ValueError(name)
    P = np.ascontiguousarray(np.stack(cols, axis=1))
    assert P.shape == (n, KIND_PARAMS[kind])
    return P


class SparseReference:
    """An independent, extended-precision solve of the global system A = M + dt^2 D^T W^2 D, assembled as a scipy.sparse matrix from the
    ORACLE's selector D (D_triplets), its weight diagonal and the masses -- not from the library's assembly (apply_A).  splu (SuperLU)
    factors it once; every solution is refined with residuals evaluated in np.longdouble until the correction is below 1e-16 of the
    solution (solve), or below the floor that the longdouble residual itself sets on an ill-conditioned system (solve_ill).  kappa1
    estimates the 1-norm condition number: onenormest of A times onenormest of A^-1 applied through the LU; kappa1_eq (lazy) is the
    same estimate for the equilibrated matrix D^-1/2 A D^-1/2, D = diag(A) -- what is left of kappa1 once bad scaling, which
    Cholesky does not feel, is taken out.

    with_weights(w) rebuilds the reference for new per-force weights (System::recompute_weights with edited Force::weight members): the
    rows of force i are [global_idx_i, global_idx_i + rows of its kind) of W, the layout the constructor checks against the oracle's W."""

    def __init__(self, oracle, m3, dt):
        import scipy.sparse as sp
        self.dt, self.m3 = float(dt), np.asarray(m3, dtype=np.float64).ravel()
        rr, cc, vv = oracle.D_triplets()
        self.n, self.rows = self.m3.size, oracle.rows
        self.D = sp.csr_matrix((vv, (rr, cc)), shape=(self.rows, self.n))
        self.kinds = np.array([oracle.force(i).kind for i in range(oracle.n_forces)])
        self.gidx = oracle.global_idx()
        self.w0 = oracle.weights()
        W = oracle.wdiag
        assert np.array_equal(self._wdiag(self.w0), W), "per-force rows of W do not match the oracle's weight diagonal"
        self._factor(W)

    def _wdiag(self, w):
        nrows = np.array(KIND_ROWS)[self.kinds]
        W = np.zeros(self.rows)
        W[np.repeat(self.gidx, nrows) + (np.arange(nrows.sum()) - np.repeat(np.cumsum(nrows) - nrows, nrows))] = np.repeat(w, nrows)
        return W

    @classmethod
    def from_selector(cls, D, W, m3, dt):
        """the reference of a system given by explicit selector triplets instead of an oracle: D = (rows, cols, values) over len(W) rows
        (duplicates summed), W the weight of every row, m3 the masses (3n).  with_weights needs an oracle's force layout and is not
        available here; rhs() builds M x_bar + dt^2 D^T W^2 (z - u) in np.longdouble."""
        import scipy.sparse as sp
        ref = cls.__new__(cls)
        ref.dt, ref.m3 = float(dt), np.asarray(m3, dtype=np.float64).ravel()
        rr, cc, vv = (np.asarray(a) for a in D)
        W = np.asarray(W, dtype=np.float64).ravel()
        ref.n, ref.rows = ref.m3.size, W.size
        ref.D = sp.csr_matrix((np.asarray(vv, dtype=np.float64), (rr, cc)), shape=(ref.rows, ref.n))
        ref.D.sum_duplicates()
        ref.kinds = ref.gidx = ref.w0 = None
        ref._factor(W)
        return ref

    def rhs(self, m_xbar, q):
        """M x_bar + dt^2 D^T W^2 q in np.longdouble (q = z - u, one entry per row; m_xbar may be longdouble)"""
        D = self.D.tocoo()
        ld = np.longdouble
        t = self.W.astype(ld) ** 2 * np.asarray(q, dtype=ld)
        b = np.zeros(self.n, dtype=ld)
        np.add.at(b, D.col, D.data.astype(ld) * t[D.row])
        return np.asarray(m_xbar, dtype=ld) + ld(self.dt) * ld(self.dt) * b

    def _factor(self, W):
        import scipy.sparse as sp
        import scipy.sparse.linalg as sla
        self.W = np.asarray(W, dtype=np.float64)
        A = (sp.diags(self.m3) + (self.dt * self.dt) * (self.D.T @ sp.diags(W * W) @ self.D)).tocsr()
        A.sum_duplicates(); A.sort_indices()
        self.A = A
        self.norm_inf = float(np.abs(A).sum(axis=1).max())
        self._Al = A.data.astype(np.longdouble)
        # A is symmetric positive definite: a symmetric fill-reducing order and diagonal pivots
        self.lu = sla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        inv = sla.LinearOperator(A.shape, matvec=self.lu.solve, rmatvec=self.lu.solve, dtype=np.float64)
        self.kappa1 = float(sla.onenormest(A) * sla.onenormest(inv))

    def with_weights(self, w):
        ref = SparseReference.__new__(SparseReference)
        ref.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("A", "norm_inf", "_Al", "lu", "kappa1", "_kappa1_eq")})
        ref._factor(ref._wdiag(np.asarray(w, dtype=np.float64)))
        return ref

    def residual(self, x, b):
        """b - A x in np.longdouble"""
        A = self.A
        prod = self._Al * np.asarray(x, dtype=np.longdouble)[A.indices]
        return np.asarray(b, dtype=np.longdouble) - np.add.reduceat(prod, A.indptr[:-1])

    def backward_error(self, x, b):
        """normwise backward error |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), the residual in longdouble"""
        return float(np.abs(self.residual(x, b)).max()) / (self.norm_inf * float(np.abs(x).max()) + float(np.abs(b).max()))

    @property
    def kappa1_eq(self):
        """kappa1 of D^-1/2 A D^-1/2, D = diag(A): the same onenormest pair, the inverse applied as D^1/2 A^-1 D^1/2 through the LU"""
        if getattr(self, "_kappa1_eq", None) is None:
            import scipy.sparse as sp
            import scipy.sparse.linalg as sla
            d = np.sqrt(self.A.diagonal())
            S = sp.diags(1.0 / d)
            inv = sla.LinearOperator(self.A.shape, matvec=lambda v: d * self.lu.solve(d * np.ravel(v)), rmatvec=lambda v: d * self.lu.solve(d * np.ravel(v)), dtype=np.float64)
            self._kappa1_eq = float(sla.onenormest((S @ self.A @ S).tocsr()) * sla.onenormest(inv))
        return self._kappa1_eq

    def _refine(self, b, max_steps, floor):
        """iterative refinement, x carried in longdouble: stops when the correction is <= max(1e-16, floor) |x|_inf, or -- with a floor --
        when two successive corrections lie within a factor 2 (it has stopped shrinking).  -> (x, steps, last correction / |x|_inf)"""
        x = self.lu.solve(np.asarray(b, dtype=np.float64)).astype(np.longdouble)
        prev = np.inf
        for step in range(1, max_steps + 1):
            r = self.residual(x, b)
            dx = self.lu.solve(r.astype(np.float64))
            x = x + dx
            corr = float(np.abs(dx).max()) / float(np.abs(x).max())
            if corr <= max(1e-16, floor) or (floor > 0.0 and corr >= 0.5 * prev):
                return x, step, corr
            prev = corr
        raise AssertionError("iterative refinement did not converge in %d steps (last correction %.3g |x|)" % (max_steps, corr))

    def solve(self, b, max_steps=10):
        """-> (x_ref, the longdouble residual of x_ref, the refinement steps taken); the correction falls below 1e-16 |x| (two steps on
        the well-conditioned systems this is for; solve_ill beyond kappa1 ~ 1e5)"""
        x, step, _ = self._refine(b, max_steps, 0.0)
        xr = x.astype(np.float64)
        return xr, self.residual(xr, b), step

    def solve_ill(self, b, max_steps=40):
        """solve for an ill-conditioned system -> (x_ref, its longdouble residual, steps, the last correction relative to |x|_inf).  The
        residual is evaluated in longdouble (eps 2^-64), so a correction cannot fall below about 2^-64 kappa1 |x|: refinement stops
        at max(1e-16, 8 * 2^-64 * kappa1) |x|, or when the correction has stopped shrinking.  The last correction bounds what is
        left of the error, up to the contraction factor (~ 2^-53 kappa1 << 1) of one more step."""
        x, step, corr = self._refine(b, max_steps, 8.0 * 2.0 ** -64 * self.kappa1)
        xr = x.astype(np.float64)
        return xr, self.residual(xr, b), step, corr


def selector_rows(oracle, f0, f1, rng=None, split=0.0):
    """the oracle's forces [f0, f1) restated as ONE generic batch (admm_hip_add_generic_batch): element e is force f0 + e, its rows
    those of the force in the oracle's order.  -> (elem_row_ptr, trip_row, trip_col, trip_val, row_weight, oracle_rows), oracle_rows[r]
    the oracle's row of batch row r.  With rng the triplets come shuffled and a fraction `split` of them as two halves (v/2 + v/2 is v
    exactly: the summed entry is the oracle's bit for bit)."""
    rr, cc, vv = oracle.D_triplets()
    gi = oracle.global_idx()
    nrows = np.array([KIND_ROWS[oracle.force(i).kind] for i in range(f0, f1)], np.int64)
    erp = np.concatenate([[0], np.cumsum(nrows)])
    orows = np.repeat(gi[f0:f1], nrows) + (np.arange(erp[-1]) - np.repeat(erp[:-1], nrows))
    bat = np.full(oracle.rows, -1, np.int64)
    bat[orows] = np.arange(orows.size)
    sel = bat[rr] >= 0
    tr, tc, tv = bat[rr[sel]], cc[sel].astype(np.int64), vv[sel]
    if rng is not None:
        half = rng.random(tr.size) < split
        tr = np.concatenate([tr[~half], tr[half], tr[half]]); tc = np.concatenate([tc[~half], tc[half], tc[half]])
        tv = np.concatenate([tv[~half], 0.5 * tv[half], 0.5 * tv[half]])
        p = rng.permutation(tr.size)
        tr, tc, tv = tr[p], tc[p], tv[p]
    return erp.astype(np.int32), tr.astype(np.int32), tc.astype(np.int32), tv, oracle.wdiag[orows], orows


def scene_reference(x, m3, forces, dt=0.04):
    """SparseReference of any scene, through the oracle: nodes x (n x 3), masses m3 (3n), forces a list of (kind name, index array,
    params) in the order the library gets them"""
    o = Oracle(); o.settings(dt, 1)
    o.add_nodes(np.asarray(x, dtype=np.float64).ravel(), m3)
    for kind, idx, params in forces:
        o.add_forces(KIND[kind], idx, params)
    assert o.initialize()
    return SparseReference(o, m3, dt)


def bar_reference(mg, dims, mu=1e5, lam=1e5, max_iter=5, density=1000.0, dt=0.04):
    """SparseReference of the bar that make_bar_system builds (Neo-Hookean tets + anchors on the k = 0 face), through the oracle"""
    x, t = mg.bar(*dims)
    m3 = np.repeat(mg.lumped_tet_mass(x, t, density), 3)
    forces = [("TET_NH", t, [mu, lam, max_iter]), ("ANCHOR", mg.bar_anchor_nodes(dims[0], dims[1]), [-1.0, 1.0])]
    return scene_reference(x, m3, forces, dt), x, m3


# ---- scenes for the elimination-tree shapes structured bars do not give (tests/test_sweep_subtree_trees.py) ----
def tet_volumes(x, t):
    a = x[t[:, 1]] - x[t[:, 0]]
    return np.einsum("ij,ij->i", a, np.cross(x[t[:, 2]] - x[t[:, 0]], x[t[:, 3]] - x[t[:, 0]])) / 6.0


def delaunay_scene(n_pts, seed=42, box=(0.6, 0.6, 6.0), stiffness=5e4, density=1000.0):
    """Delaunay tets of n_pts random points in a long box, slivers (quality 6 sqrt(2) volume / longest edge^3 <= 0.05) dropped, every
    point still used; corotational tets, lumped masses, the points below z = 0.15 anchored -> (x, m3, forces).  The points are numbered
    along the box (sorted by z): the oracle factors in natural order, and a band as narrow as a structured bar's keeps its fill alike."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, size=(n_pts, 3)) * np.array(box)
    x = x[np.argsort(x[:, 2], kind="stable")]
    t = Delaunay(x).simplices.astype(np.int32)
    v = np.abs(tet_volumes(x, t))
    lmax = np.stack([np.linalg.norm(x[t[:, i]] - x[t[:, j]], axis=1) for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))], axis=1).max(axis=1)
    keep = 6.0 * np.sqrt(2.0) * v > 0.05 * lmax ** 3      # (1 for a regular tet; slivers would take kappa1 to ~1e9)
    t, v = t[keep], v[keep]
    assert np.unique(t).size == n_pts
    m = np.zeros(n_pts)
    np.add.at(m, t.ravel(), np.repeat(v * density / 4.0, 4))
    anchors = np.nonzero(x[:, 2] < 0.15)[0].astype(np.int32)
    return x, np.repeat(m, 3), [("TET_LINEAR", t, [stiffness]), ("ANCHOR", anchors, [-1.0, 1.0])]


def forest_scene(mg, n_small=400, big=(16, 16, 40), seed=5, stiffness=5e4, density=1000.0):
    """n_small disconnected little bars of 1 x 1 x 1 up to 3 x 3 x 4 cells on a grid beside one larger bar, all in one system:
    nested dissection splits between bodies (empty separators), so the elimination tree gets supernodes with no contribution rows
    under a parent.  Corotational tets, lumped masses, the big bar's k = 0 face anchored -> (x, m3, forces)"""
    rng = np.random.default_rng(seed)
    xs, ts, off = [], [], 0
    x, t = mg.bar(*big)
    xs.append(x); ts.append(t); off = x.shape[0]
    anchors = mg.bar_anchor_nodes(big[0], big[1])
    side = int(np.ceil(np.sqrt(n_small)))
    for b in range(n_small):
        dims = (int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 5)))
        x, t = mg.bar(*dims)
        x = x + np.array([1.5 + 0.3 * (b % side), 0.3 * (b // side), 0.0])
        xs.append(x); ts.append(t + off); off += x.shape[0]
    x, t = np.concatenate(xs), np.concatenate(ts).astype(np.int32)
    m3 = np.repeat(mg.lumped_tet_mass(x, t, density), 3)
    return x, m3, [("TET_LINEAR", t, [stiffness]), ("ANCHOR", anchors, [-1.0, 1.0])]


def scene_system(pkg, x, m3, forces, dt=0.04, device_id=0, rank=0, world=1):
    """the library's System of a scene of delaunay_scene / forest_scene (gravity added), not yet initialized"""
    s = pkg.System(device_id=device_id); s.set_timestep(dt)
    s.add_nodes(np.asarray(x, dtype=np.float64).ravel(), m3)
    for kind, idx, params in forces:
        s.add_forces(pkg.KIND[kind], idx, params)
    s.add_gravity([0.0, -9.8, 0.0])
    if world > 1:
        s.set_shard(rank, world)
        s.set_shard_mode("subtree")
    return s


# ---- per-iteration ADMM residuals recomputed from captured states (tests/test_residual_reference.py) ----
EPS = 2.0 ** -53      # unit roundoff of binary64: every device operation below is x (1 + d), |d| <= EPS


def gamma(k):
    """Higham's gamma_k = k EPS / (1 - k EPS): k roundings in a row"""
    return k * EPS / (1.0 - k * EPS)


class ResidualReference:
    """The primal and dual residual of ONE ADMM iteration j, recomputed in np.longdouble from states captured on both sides of it, in the
    oracle's definitions (orc_step; the comment at System.cpp:64-65):

        r_j = | W (D x_j - z_{j+1}) |           = | W (u_{j+1} - u_j) |   since every kind updates u += D x - z
        s_j = | D^T W^2 (z_{j+1} - zprev_j) |   zprev_0 = D m_x at the frame's start, zprev_j = z_j afterwards

    D (compact row layout) and W are the ORACLE's (D_triplets, wdiag: pinned to the compiled reference by test_oracle_vs_ref.py); nothing here
    calls the library under test.  All vectors are in the oracle's row order; rows_of() maps a batch's per-element [n][rows] arrays there.
    Every method takes `drop`, a boolean mask over the rows left out of the sums (the sensitivity condition: one element removed).

    The longdouble arithmetic (eps <= 2^-63, asserted) contributes errors 1000 times below anything bounded here and is not counted.

    Error bounds, from the kernels' operation counts (EPS = 2^-53, gamma_k = k EPS / (1 - k EPS)); nothing measured goes into them:

    |r_dev - r_from_u| <= c_r EPS r_from_u.  Per row the device forms du = fl(u_new - u_old) from the very doubles the reference subtracts
      exactly (1 rounding), squares it (du^2: 2 + 1), adds the element's `rows` squares from 0 (rows - 1 inexact additions), multiplies by
      w^2 = fl(w w) (1 + 1), then sums non-negative terms: the in-block reduction (6 levels of the 64-lane butterfly in the fused tet / anchor
      kernels, 8 levels of the 256-entry tree in residual_primal_kernel: 8 covers both), sum_partials_kernel's strided serial part
      (ceil(partials / 256) - 1 additions, partials = ceil(elements / elements per block) of the largest batch), its 256-entry tree (8), one
      addition per further batch (the accumulate flag) and per further rank (the all-reduce).  For a sum of non-negative terms the relative
      error is bounded by the deepest chain: C2 = 3 + (rows - 1) + 2 + 8 + serial + 8 + (batches - 1) + (ranks - 1) roundings in r^2.  The square
      root halves that and adds its own rounding; one more unit absorbs the second-order terms:  c_r = ceil(C2 / 2) + 2  (c_r(): C2 = 29 -> 17 for a
      lone 9-row batch and C2 = 30 -> 17 with its anchors, 18 on two ranks, 20 for the seven batches of the mixed scene, 17 + 1 per two
      serial additions; every test prints the c_r, c_s and serial count it used).

    |r_dev - r_from_dx| <= the above + 2 EPS |W u_{j+1}| + gamma_nnz |W |D| |x_j||.  The device's u_new = fl(u + fl(Dx_dev - z)) differs from
      u + (D x - z) by the rounding of the sum (EPS |u_new|), of the difference (EPS |Dx - z| <= EPS (|u_new| + |u_old|), of which |u_new - u_old|
      is already inside c_r) and of its own D x (nnz products and nnz - 1 additions per row: gamma_nnz |D||x|); the triangle inequality
      carries the row-wise terms to the weighted norms.

    |s_dev - s_ref| <= gamma_m | |D^T| W^2 |z_{j+1} - zprev_j| | + c_s EPS s_ref,   m = entries per selector row + largest node degree + 2.
      Per corner the device rounds dz = fl(z - zprev), w^2, w^2 dz, every product with the selector entry and the additions of the element's
      `cols` <= 3 products; the corner shares of a node then meet in at most (degree - 1) inexact additions (pre-reduced layout: the block's run
      in LDS plus the node's slots; per-corner layout: the node's slots; sharded: plus one per further rank) -- `degree` counts every corner of
      every element on the node.  c_s: the square (1), the gather's / norm2_partial_kernel's 256-entry tree (8), sum_partials_kernel's serial
      part and tree (serial + 8): C2 = 17 + serial, c_s = ceil(C2 / 2) + 2.
      At j = 0 the device's own warm start fl(D m_x) (residual_dx_kernel: gamma_nnz |D||m_x| per row) stands in for D m_x:
      + gamma_nnz | |D^T| W^2 |D| |m_x| |."""

    def __init__(self, oracle):
        ld = np.longdouble
        assert np.finfo(ld).eps <= 2.0 ** -63, "np.longdouble has no extended precision here (the tests that use this skip on such hosts)"
        rr, cc, vv = oracle.D_triplets()
        self.rows, self.n = oracle.rows, oracle.dof
        self.rr, self.cc, self.vv = rr.astype(np.int64), cc.astype(np.int64), vv.astype(ld)
        self.W = oracle.wdiag.astype(ld)
        self.kinds = np.array([oracle.force(i).kind for i in range(oracle.n_forces)])
        self.gidx = oracle.global_idx()
        self.weights = oracle.weights()
        self.nrows = np.array(KIND_ROWS)[self.kinds]
        self.row_force = np.full(self.rows, -1, np.int64)
        self.row_force[np.repeat(self.gidx, self.nrows) + (np.arange(self.nrows.sum()) - np.repeat(np.cumsum(self.nrows) - self.nrows, self.nrows))] = np.repeat(np.arange(self.kinds.size), self.nrows)
        assert (self.row_force >= 0).all()
        self.nnz_row = int(np.bincount(rr, minlength=self.rows).max())
        # degree: corners of elements on a node = distinct (force, node) pairs
        pairs = np.unique(np.stack([self.row_force[rr], cc // 3]), axis=1)
        self.max_degree = int(np.bincount(pairs[1]).max())

    # -- layout --
    def rows_of(self, first_force, elements, kind):
        """oracle rows [len(elements)][rows of kind] of a batch's elements (ids inside the batch, e.g. local_elements of a rank); first_force =
        the oracle's force index of the batch's element 0"""
        f = first_force + np.asarray(elements, dtype=np.int64)
        assert (self.kinds[f] == kind).all()
        return self.gidx[f][:, None] + np.arange(KIND_ROWS[kind])[None, :]

    def force_rows(self, force):
        return np.arange(self.gidx[force], self.gidx[force] + self.nrows[force])

    def _keep(self, drop):
        return np.ones(self.rows, bool) if drop is None else ~np.asarray(drop, bool)

    def _D(self, x, absolute=False):
        ld = np.longdouble
        out = np.zeros(self.rows, ld)
        xv = np.asarray(x, dtype=ld)
        np.add.at(out, self.rr, (np.abs(self.vv) * np.abs(xv[self.cc])) if absolute else self.vv * xv[self.cc])
        return out

    def _DT(self, q, absolute=False):
        ld = np.longdouble
        out = np.zeros(self.n, ld)
        qv = np.asarray(q, dtype=ld)
        np.add.at(out, self.cc, (np.abs(self.vv) * np.abs(qv[self.rr])) if absolute else self.vv * qv[self.rr])
        return out

    @staticmethod
    def _norm(v):
        return np.sqrt(np.sum(v * v))

    # -- the residuals --
    def r_from_u(self, u0, u1, drop=None):
        ld = np.longdouble
        d = self.W * (np.asarray(u1, dtype=ld) - np.asarray(u0, dtype=ld))
        return self._norm(d[self._keep(drop)])

    def r_from_dx(self, x, z1, drop=None):
        d = self.W * (self._D(x) - np.asarray(z1, dtype=np.longdouble))
        return self._norm(d[self._keep(drop)])

    def zprev_frame_start(self, x):
        return self._D(x)

    def s(self, z1, zprev, drop=None):
        ld = np.longdouble
        q = self.W * self.W * (np.asarray(z1, dtype=ld) - np.asarray(zprev, dtype=ld))
        q[~self._keep(drop)] = 0
        return self._norm(self._DT(q))

    # -- the bounds --
    def serial(self, partials):
        """additions in sum_partials_kernel's strided serial part: ceil(count / 256) - 1 over the longest array it sums -- `partials`, the most
        partials any batch leaves (one per block of its projection kernel or of residual_primal_kernel), or the 256-entry blocks of the 3n-vector s"""
        part = max(int(partials), -(-self.n // 256))
        return max(-(-part // 256) - 1, 0)

    def c_r(self, batches=1, serial=0, ranks=1):
        c2 = 3 + (int(self.nrows.max()) - 1) + 2 + 8 + serial + 8 + (batches - 1) + (ranks - 1)
        return -(-c2 // 2) + 2

    def c_s(self, serial=0):
        return -(-(17 + serial) // 2) + 2

    def bound_r_u(self, u0, u1, c_r):
        return float(c_r * EPS * self.r_from_u(u0, u1))

    def bound_r_dx(self, x, u0, u1, c_r):
        ld = np.longdouble
        extra = 2 * EPS * self._norm(self.W * np.asarray(u1, dtype=ld)) + gamma(self.nnz_row) * self._norm(self.W * self._D(x, absolute=True))
        return self.bound_r_u(u0, u1, c_r) + float(extra)

    def bound_s(self, z1, zprev, c_s, x_start=None, ranks=1):
        """x_start: the frame's m_x when zprev is the warm start D m_x (iteration 0), None otherwise"""
        ld = np.longdouble
        m = self.nnz_row + self.max_degree + 2 + (ranks - 1)
        w2 = self.W * self.W
        b = gamma(m) * self._norm(self._DT(w2 * np.abs(np.asarray(z1, dtype=ld) - np.asarray(zprev, dtype=ld)), absolute=True))
        if x_start is not None:
            b = b + gamma(self.nnz_row) * self._norm(self._DT(w2 * self._D(x_start, absolute=True), absolute=True))
        return float(b + c_s * EPS * self.s(z1, zprev))


# ---- the assembled right-hand side recomputed from captured states (tests/test_rhs_reference.py) ----
class RhsReference(ResidualReference):
    """The right-hand side of the global step, b = M x_bar + dt^2 D^T W^2 (z - u), recomputed in np.longdouble from the u and z a local step
    left behind (the states AFTER it, in the oracle's row order; rows_of() maps a batch's per-element arrays there).  D (compact rows), W and
    the masses are the ORACLE's (D_triplets, wdiag, the m3 it was given); nothing here calls the library under test.

    A `corner` is one (force, node) pair: the node's share of one element, dt^2 sum_r D[r, 3 node + j] w_r^2 (z - u)_r for j = 0..2.
    corner_force / corner_node name them, degree[node] counts the corners on a node, b(drop=...) leaves corners out (the sensitivity
    condition: one share dropped moves b by exactly that share).

    bound(): |b_dev - b_ref| <= gamma_k (|m x_bar| + dt^2 |D^T| W^2 |z - u|) per dof, k from the kernels' operation counts (EPS = 2^-53,
    gamma_k = k EPS / (1 - k EPS)); nothing measured goes into it:
      * q = fl(z - u_new): the device's u_new and z are the very doubles the reference reads back, so this is ONE rounding              1
      * the factor dt^2 w^2 = fl(fl(dt dt) fl(w w)) (w2h2 of upload.inc)                                                                3
      * the product with the selector entry and the product with that factor -- s (B q) in the tet and triangle kernels, s q alone
        where the entry is +-1 (anchors, collisions, springs, hinges): at most                                                          2
      * the additions of one corner's terms, T - 1 with T = the most entries one element has in one column of D (3 for tets, 2 for
        triangles, 1 otherwise; the hinge's minus-all corner adds 2: its three terms count as T = 3 there)                             T - 1
      * the corners of a node meet in at most (corners on the node - 1) additions whichever layout and block cut is used: the run in the
        block's LDS staging plus the node's slots in the gather never exceed it                                                  degree - 1
      * the addition of fl(m x_bar) (its own product rounding and this addition stay below the count of the other terms)                1
    k(node) = 7 + (T - 1) + (degree(node) - 1).  The ranks' vectors of a sharded context are summed in np.longdouble by the test: every rank
    adds fewer corners than the node has, M x_bar enters on one rank, and the same bound holds.
    The longdouble arithmetic (eps <= 2^-63, asserted) contributes errors 1000 times below this and is not counted."""

    def __init__(self, oracle, dt=0.04):
        super().__init__(oracle)
        ld = np.longdouble
        self.dt = float(dt)
        self.m3 = np.asarray(oracle.m3, dtype=np.float64)
        assert self.m3.size == self.n
        force, node = self.row_force[self.rr], self.cc // 3
        key, self.entry_corner = np.unique(force * (self.n // 3) + node, return_inverse=True)
        self.corner_force, self.corner_node = key // (self.n // 3), key % (self.n // 3)
        self.n_corners = key.size
        self.degree = np.bincount(self.corner_node, minlength=self.n // 3)
        T = int(np.bincount(self.entry_corner * 3 + self.cc % 3).max())
        if (self.kinds == KIND["BEND"]).any():
            T = max(T, 3)
        self.T = T
        self.k_dof = np.repeat(7 + (T - 1) + np.maximum(self.degree - 1, 0), 3)
        self._coef = ld(self.dt) * ld(self.dt) * self.vv * (self.W * self.W)[self.rr]      # dt^2 D[r, c] w_r^2 per entry

    def shares(self, u, z, absolute=False):
        """[corners][3]: every corner's share of b (absolute: of |D^T| W^2 |z - u|)"""
        ld = np.longdouble
        q = np.asarray(z, dtype=ld) - np.asarray(u, dtype=ld)
        t = self._coef * q[self.rr]
        out = np.zeros(3 * self.n_corners, ld)
        np.add.at(out, self.entry_corner * 3 + self.cc % 3, np.abs(t) if absolute else t)
        return out.reshape(-1, 3)

    def _scatter(self, sh, drop=None):
        out = np.zeros(self.n, np.longdouble)
        keep = np.ones(self.n_corners, bool) if drop is None else ~np.asarray(drop, bool)
        dof = (3 * self.corner_node[keep])[:, None] + np.arange(3)[None, :]
        np.add.at(out, dof.ravel(), sh[keep].ravel())
        return out

    def b(self, xbar, u, z, drop=None):
        """drop: a boolean mask over the corners left out"""
        ld = np.longdouble
        return self.m3.astype(ld) * np.asarray(xbar, dtype=ld) + self._scatter(self.shares(u, z), drop)

    def bound(self, xbar, u, z):
        ld = np.longdouble
        mag = np.abs(self.m3.astype(ld) * np.asarray(xbar, dtype=ld)) + self._scatter(self.shares(u, z, absolute=True))
        k = self.k_dof.astype(ld)
        return (k * EPS / (1.0 - k * EPS)) * mag

    def corner_sensitivity(self, xbar, u, z):
        """per corner: by how many bounds its removal moves b in its most sensitive component"""
        bd = self.bound(xbar, u, z).reshape(-1, 3)
        return np.max(np.abs(self.shares(u, z)) / bd[self.corner_node], axis=1).astype(np.float64)


# ---- the explicit forces of a frame in np.longdouble (tests/test_explicit_reference.py) ----
def _explicit(x, v, dt, forces, with_bound):
    ld = np.longdouble
    assert np.finfo(ld).eps <= 2.0 ** -63, "np.longdouble has no extended precision here (the tests that use this skip on such hosts)"
    X = np.asarray(x, dtype=np.float64).reshape(-1, 3).astype(ld)
    V = np.asarray(v, dtype=np.float64).reshape(-1, 3).astype(ld).copy()
    n = X.shape[0]
    h = ld(float(dt))
    E = np.zeros((n, 3), ld)      # running first-order bound on the device's error in v
    e = ld(EPS)
    third, c33, k1000 = ld(3.0), ld(0.33), ld(1000.0)      # the doubles the kernels hold (0.33 is not exact: the same double here)
    P, Q = [1, 2, 0], [2, 0, 1]
    for type_, direction, idx in forces:
        d = np.asarray(direction, dtype=np.float64).astype(ld)
        if type_ == "const":
            sel = np.arange(n) if idx is None or len(idx) == 0 else np.asarray(idx, dtype=np.int64)      # an empty list = every node (ExplicitForce.cpp:30-32)
            inc = h * d
            for node in (sel if np.unique(sel).size != sel.size else [sel]):      # (a list naming a node twice increments it twice)
                V[node] += inc
                if with_bound:
                    E[node] += e * np.abs(inc) + e * np.abs(V[node])
            continue
        assert type_ == "wind"
        tris = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
        # the geometry reads x only: all triangles at once
        a, b = X[tris[:, 1]] - X[tris[:, 0]], X[tris[:, 2]] - X[tris[:, 0]]
        nv = a[:, P] * b[:, Q] - a[:, Q] * b[:, P]
        nn = np.sqrt(nv[:, 0] * nv[:, 0] + (nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2]))
        nm = nv / nn[:, None]
        area = ld(0.5) * nn
        if with_bound:
            dn = 4 * e * (np.abs(a[:, P] * b[:, Q]) + np.abs(a[:, Q] * b[:, P]))
            dnn = (np.abs(nv) * dn).sum(axis=1) / nn + 3 * e * nn
            dnm = dn / nn[:, None] + np.abs(nm) * (dnn / nn)[:, None] + e * np.abs(nm)
            darea = ld(0.5) * dnn
        for t in range(tris.shape[0]):      # serial triangle order: each triangle sees the velocities the earlier ones left
            i = tris[t]
            vv = V[i]
            vr = (vv[0] + vv[1] + vv[2]) / third - d
            vn = (nm[t] * vr).sum()
            c = -k1000 * area[t] * vn * abs(vn)
            f = c * nm[t] * c33 * h
            if with_bound:
                dvr = E[i].sum(axis=0) / 3 + e * (np.abs(vv).sum(axis=0) + np.abs(vr))
                dvn = (dnm[t] * np.abs(vr) + np.abs(nm[t]) * dvr).sum() + 3 * e * np.abs(nm[t] * vr).sum()
                dc = k1000 * (darea[t] * vn * vn + 2 * area[t] * abs(vn) * dvn) + 3 * e * abs(c)
                df = c33 * h * (dc * np.abs(nm[t]) + abs(c) * dnm[t]) + 3 * e * np.abs(f)
            for q in range(3):      # corner by corner: a triangle naming one node twice increments it twice
                V[i[q]] += f
                if with_bound:
                    E[i[q]] += df + e * np.abs(V[i[q]])
    xbar = X + h * V
    vout = (xbar - X) * (ld(1.0) / h)
    out = (xbar.ravel(), vout.ravel(), V.ravel())
    if not with_bound:
        return out
    bx = h * E + e * np.abs(h * V) + e * np.abs(xbar)
    bvout = bx / h + 3 * e * np.abs(vout)
    second = ld(1.0) + ld(2.0) ** -10      # the neglected products of two errors, each below 1e-13 of a first-order term
    return out, (second * bx.ravel(), second * bvout.ravel(), second * E.ravel())


def explicit_reference(x, v, dt, forces):
    """The explicit part of a frame (System.cpp:37-48, 70-71 with no ADMM iteration in between) in np.longdouble, the forces in LIST ORDER.
    forces: [("const", g, idx or None), ("wind", direction, tris)].  A constant force adds dt g on all nodes (idx None or empty:
    ExplicitForce.cpp:30-32) or on a subset.  The wind (ExplicitForce.cpp:42-98 as wind_serial_kernel's comment states it) runs in SERIAL
    triangle order: each triangle sees the velocities the earlier ones left, v_r = (v_0 + v_1 + v_2) / 3 - direction, n = a x b with
    a = x_1 - x_0, b = x_2 - x_0, normal = n / |n|, area = |n| / 2, v_n = normal . v_r, force = -1000 area v_n |v_n| normal, times 0.33, times dt,
    added to each of the triangle's three corners in turn.  Then x_bar = x + dt v' and v_out = (x_bar - x) (1 / dt).  -> (x_bar, v_out, v')."""
    return _explicit(x, v, dt, forces, False)


def explicit_bound(x, v, dt, forces):
    """-> ((x_bar, v_out, v'), (bound on the device's x_bar, on its v_out, on its v')): a running first-order bound of the device's rounding
    errors against explicit_reference, from the kernels' operations (EPS = 2^-53 each; nothing measured goes into it):
      * a constant force, v = fl(v + fl(dt g)): TWO roundings per force on the node, EPS |dt g| + EPS |v|;
      * the wind, per triangle: a, b one rounding each; every component of a x b two products and a subtraction on them, 4 EPS (|a_p b_q| +
        |a_q b_p|); |n| its squares, two additions and the root, 3 EPS |n| on top of what n carries; normal = n / |n| one more; v_r two
        additions, a division and a subtraction, EPS (|v_0| + |v_1| + |v_2| + |v_r|) on top of a third of the three nodes' carried bounds
        (this is how the serial chain through a node propagates); v_n three products and two additions, 3 EPS sum |normal_j v_r,j|; the
        coefficient -1000 area v_n |v_n| three products; the force three more (normal, 0.33, dt); and each of the three increments one
        rounding, EPS |v| -- once per triangle on the node;
      * x_bar = fl(x + fl(dt v')): TWO more, dt bound(v') + EPS |dt v'| + EPS |x_bar|;
      * v_out = fl(fl(x_bar - x) fl(1 / dt)): the subtraction, the reciprocal and the product, bound(x_bar) / dt + 3 EPS |v_out| -- the
        EPS |x_bar| / dt inside the first term dominates everything else.
    The products of two errors are covered by a factor 1 + 2^-10."""
    return _explicit(x, v, dt, forces, True)


# ---- a caller's non-blocking stream with skewed queues (tests/test_caller_stream.py) ------------------------------------------------
HIP_STREAM_NON_BLOCKING = 0x01


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's copy, which libadmm_hip.so binds to as well), as a ctypes handle: the
    path comes from the process's own mappings, and opening a path that is already mapped returns the loaded image -- no second runtime."""
    import torch
    torch.cuda.init()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line and "r-xp" in line})
    assert len(paths) == 1, "expected exactly one HIP runtime in this process: %r" % (paths,)
    rt = C.CDLL(paths[0])
    rt.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    rt.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    return rt


def stream_flags(stream):
    """hipStreamGetFlags of a torch stream"""
    fl = C.c_uint(0xFFFF)
    rc = hip_runtime().hipStreamGetFlags(C.c_void_p(stream.cuda_stream), C.byref(fl))
    assert rc == 0, "hipStreamGetFlags failed (%d)" % rc
    return fl.value


def nonblocking_stream():
    """-> (a torch stream that has no implicit ordering with the legacy default stream, its flags as read back).  torch's pool
    streams are created non-blocking; should a build hand out a blocking one, a stream is created with hipStreamNonBlocking through
    the same runtime and wrapped (it lives as long as the process: the tests' streams are module fixtures)."""
    import torch
    st = torch.cuda.Stream()
    if not stream_flags(st) & HIP_STREAM_NON_BLOCKING:
        h = C.c_void_p()
        rc = hip_runtime().hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING)
        assert rc == 0 and h.value, "hipStreamCreateWithFlags failed (%d)" % rc
        st = torch.cuda.ExternalStream(h.value)
    fl = stream_flags(st)
    assert st.cuda_stream != 0 and fl & HIP_STREAM_NON_BLOCKING, (st.cuda_stream, fl)
    return st, fl


class Delay:
    """A kernel that keeps a queue busy for 5 to 20 ms: torch.cuda._sleep, or a fixed stack of matrix products should that not land in
    the window; its length is calibrated once with events (aim: 8 ms) and measured again -- .ms is that last measurement."""
    LO_MS, HI_MS, AIM_MS = 5.0, 20.0, 8.0

    def __init__(self):
        import torch
        self.torch = torch
        self.a = None
        for kind in ("sleep", "matmul"):
            self.kind = kind
            if kind == "matmul":
                self.a = torch.randn(1024, 1024, device="cuda")
            self.n = 2_000_000 if kind == "sleep" else 8
            self._measure(); first = self._measure()                 # (the first launch pays for loading the kernel)
            self.ms = first
            for _ in range(3):                                        # (a second and third scaling only if a measurement was disturbed)
                self.n = max(1, int(round(self.n * self.AIM_MS / max(self.ms, 1e-3))))
                self.ms = self._measure()
                if self.LO_MS + 1.0 <= self.ms <= self.HI_MS - 5.0:
                    break
            if self.LO_MS <= self.ms <= self.HI_MS:
                break
        assert self.LO_MS <= self.ms <= self.HI_MS, "no delay kernel between %g and %g ms (%s: %.2f ms)" % (self.LO_MS, self.HI_MS, self.kind, self.ms)

    def _measure(self):
        t = self.torch
        st = t.cuda.current_stream()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        t.cuda.synchronize()
        e0.record(st); self(st); e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self, stream):
        t = self.torch
        with t.cuda.stream(stream):
            if self.kind == "sleep":
                t.cuda._sleep(self.n)
            else:
                b = self.a
                for _ in range(self.n):
                    b = b @ self.a * (1.0 / 32.0)


class Skew:
    """Keeps one queue busy in front of every library call.  mode None: nothing; "A": the delay goes on the caller's stream (the call's
    own work queues behind it: a host read, overwrite or free that does not wait for the context's stream sees the state before the
    call); "B": on the legacy default stream (work the library leaves there runs late, unordered against the context's stream).
    Armed after set-up.  before() asserts that the delay is still running when the call begins and counts the call."""

    def __init__(self, mode, stream, delay):
        import torch
        assert mode in (None, "A", "B")
        self.torch, self.mode, self.delay, self.armed, self.calls = torch, mode, delay, False, 0
        self.queue = None if mode is None else (stream if mode == "A" else torch.cuda.default_stream())

    def arm(self):
        self.armed = True

    def before(self, name=""):
        if self.mode is None or not self.armed:
            return
        self.delay(self.queue)
        ev = self.torch.cuda.Event()
        ev.record(self.queue)
        assert not ev.query(), "skew %s: call %d (%s) began on an idle queue" % (self.mode, self.calls, name)
        self.calls += 1


class Skewed:
    """A System whose calls that reach the device are each preceded by skew.before(); attributes and host-only calls pass through."""
    HOST_ONLY = frozenset(("graph_state", "info", "collision_form", "read_rest", "local_elements", "local_range", "apply_A", "n_collision_shapes",
                           "node_owner", "node_supernode"))

    def __init__(self, system, skew):
        object.__setattr__(self, "raw", system)
        object.__setattr__(self, "skew", skew)

    def __getattr__(self, name):
        s, skew = self.raw, self.skew
        if isinstance(getattr(type(s), name, None), property):
            skew.before(name)
            return getattr(s, name)
        v = getattr(s, name)
        if not callable(v) or name in self.HOST_ONLY:
            return v

        def call(*a, **k):
            skew.before(name)
            return v(*a, **k)
        return call

    def __setattr__(self, name, val):
        if isinstance(getattr(type(self.raw), name, None), property):
            self.skew.before(name + " =")
        setattr(self.raw, name, val)


def same_bits(a, b):
    """np.array_equal through lists, tuples and dicts (NaNs equal: a NaN is a value here); anything else by =="""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(p, q) for p, q in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


def stream_ordered_allreduce_hooks(world):
    """all-reduce between `world` contexts in ONE process on ONE GPU that never synchronises the device: every rank records a "ready"
    event on the stream it is handed; rank 0's stream waits for all of them, sums (rank order, like the synchronising test hooks) and
    writes every rank's buffer, then records "done", which the other ranks' streams wait for.  The host threads meet at two barriers.
    -> (hooks, calls: how often every rank's hook has run)"""
    import threading
    import torch
    bar = threading.Barrier(world)
    bufs, ready, done, calls = {}, {}, {}, [0] * world

    class _Ptr:
        def __init__(self, ptr, count):
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2}

    def make_hook(r):
        def hook(ptr, count, stream):
            assert stream, "the hook was handed the legacy default stream"
            st = torch.cuda.ExternalStream(stream)
            bufs[r] = torch.as_tensor(_Ptr(ptr, count), device="cuda:0")
            ready[r] = torch.cuda.Event()
            ready[r].record(st)
            bar.wait(timeout=120)
            if r == 0:
                for q in range(world):
                    st.wait_event(ready[q])
                with torch.cuda.stream(st):
                    tot = bufs[0].clone()
                    for q in range(1, world):
                        tot += bufs[q]
                    for q in range(world):
                        bufs[q].copy_(tot)
                done[0] = torch.cuda.Event()
                done[0].record(st)
            bar.wait(timeout=120)
            if r != 0:
                st.wait_event(done[0])
            calls[r] += 1
            return 0
        return hook
    return [make_hook(r) for r in range(world)], calls
