"""admm-elastic-sca_amd: MI355X-native ADMM elastic solver (hot path of
mattoverby/admm-elastic-sca) -- Python plumbing over the C ABI.

The product is libadmm_hip.so (HIP kernels + C ABI, include/admm_hip.h).  This
module only binds it with ctypes for bench.py / tests and mirrors the
reference's ``admm::System`` surface (``add_nodes``, ``forces``, ``initialize``,
``step``, ``m_x``/``m_v``; reference deps/admm-elastic-sca/src/system/System.hpp:29-76)
so that scene code reads like the reference's samples.  There is no CPU
fallback: without the library or without a GPU every compute call raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build
from . import meshgen  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libadmm_hip.so")

KIND = dict(ANCHOR=0, SPRING=1, TET_LINEAR=2, TET_VOLUME=3, TET_NH=4, TET_STVK=5, TRI_STRAIN=6, BEND=7, COLLISION=8, TRI_AREA=9, TRI_FUNG=10)
SHARD = dict(contiguous=0, subtree=1)
# System.debug_math: op -> doubles per record (in, out); the ops' names
DEBUG_MATH_SHAPES = {0: (1, 1), 1: (1, 1), 2: (1, 1), 3: (1, 1), 4: (1, 1), 5: (2, 1), 6: (9, 21), 7: (9, 21), 8: (6, 12), 9: (12, 9)}
DEBUG_MATH_OP = dict(log=0, exp=1, sqrt_in_1_4=2, sqrt_ge_1=3, rcp_in_1_2=4, eig_hypot=5, svd3=6, oriented_svd=7, svd32=8, mt_cstep=9)
KIND_NODES = [1, 2, 4, 4, 4, 4, 3, 4, 1, 3, 3]
KIND_ROWS = [3, 3, 9, 9, 9, 9, 6, 9, 3, 6, 6]
KIND_PARAMS = [2, 1, 1, 3, 3, 3, 4, 1, 1, 4, 3]
KIND_STATE = [0, 0, 0, 0, 4, 4, 0, 0, 0, 0, 4]
SHAPE = dict(FLOOR=0, SPHERE=1, CYLINDER=2, MESH=3, BOX=4)
SHAPE_BOX = SHAPE["BOX"]
EXPLICIT = dict(CONST=0, WIND=1)
PRESSURE = {"CONSTANT": 0, "GAS": 1}      # ADMM_PRESSURE_* (include/admm_hip.h)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
PROJECT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_int64, _dp, _dp, _dp)
KIND_GENERIC = 11


class Info(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_nodes", "n_elems_total", "n_elems_local", "rows_compact", "nnz_A", "nnz_L",
                                         "panel_bytes", "n_supernodes", "n_levels", "max_super_cols", "max_super_rows",
                                         "solve_contrib_rows")] + \
               [(n, C.c_double) for n in ("t_order_s", "t_symbolic_s", "t_numeric_s", "t_upload_s")] + \
               [(n, C.c_int32) for n in ("rank", "world", "device_id", "host_threads", "dense_solve", "device_factor")] + \
               [(n, C.c_int64) for n in ("rhs_slots", "sweep_entries_own", "sweep_entries_top", "sweep_entries_top_bwd", "nodes_own", "nodes_top",
                                         "comm_doubles_iter", "comm_doubles_frame", "factor_doubles_resident", "front_doubles",
                                         "factor_exchange_doubles")] + \
               [(n, C.c_int32) for n in ("factor_local", "dist_top")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Timing(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("prologue_ms", "local_ms", "rhs_ms", "allreduce_ms", "solve_fwd_ms", "solve_bwd_ms",
                                         "epilogue_ms", "total_ms")] + [("iters", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class EnergyTotals(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("kinetic", "gravity", "elastic", "anchor")] + [(n, C.c_int64) for n in ("n_infinite", "batches_skipped")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ForceInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_nonfinite", "batches_skipped")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ReactionInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("batches_collision", "batches_anchor", "batches_skipped", "n_contacts")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# admm_hip_contact: 64 bytes, the four bytes behind `node` are padding
CONTACT_DTYPE = np.dtype(dict(names=["node", "f", "point", "depth"], formats=[np.int32, (np.float64, 3), (np.float64, 3), np.float64],
                              offsets=[0, 8, 32, 56], itemsize=64))
# admm_hip_contact_owner: 64 bytes
CONTACT_OWNER_DTYPE = np.dtype(dict(names=["node", "entry", "normal", "f_normal", "f_tangent"], formats=[np.int32, np.int32, (np.float64, 3), np.float64, (np.float64, 3)],
                                    offsets=[0, 4, 8, 32, 40], itemsize=64))
# admm_hip_surface_contact (two-way contact): status as in SURFACE_STATUS
SURFACE_CONTACT_DTYPE = np.dtype(dict(names=["node", "mesh", "tri", "corner", "status", "weight", "share"],
                                      formats=[np.int32, np.int32, np.int32, (np.int32, 3), np.int32, (np.float64, 3), np.float64],
                                      offsets=[0, 4, 8, 12, 24, 32, 56], itemsize=64))
SURFACE_STATUS = dict(reacting=0, unowned=1, other=2, self=3)


class SurfaceReactionInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_contacts", "n_reacting", "n_unowned", "n_other", "n_self")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RigidStateRecord(C.Structure):
    """admm_hip_rigid_state: a rigid body's state c, q = (w, x, y, z), v, L; derived omega, R (row-major), the entry's par; the last
    frame's applied F, tau and number of contacts"""
    _fields_ = [("c", C.c_double * 3), ("q", C.c_double * 4), ("v", C.c_double * 3), ("L", C.c_double * 3), ("omega", C.c_double * 3), ("R", C.c_double * 9),
                ("par", C.c_double * 4), ("F", C.c_double * 3), ("tau", C.c_double * 3), ("count", C.c_int64), ("entry", C.c_int32), ("pad_", C.c_int32)]


RIGID_FIELDS = ("c", "q", "v", "L", "omega", "R", "par", "F", "tau")


class RigidState:
    """one body's record as numpy arrays (c, q, v, L, omega, R [3][3], par, F, tau), count, entry; `body`: the constants rigid_query takes
    (type, mass, inertia, accel, c0, par0), None when built by hand.  frame / motion: the entry's rows of the shape table."""

    def __init__(self, rec, body=None):
        for n in RIGID_FIELDS:
            setattr(self, n, np.array(getattr(rec, n)[:], dtype=np.float64))
        self.R = self.R.reshape(3, 3)
        self.count, self.entry, self.body = int(rec.count), int(rec.entry), body

    def record(self):
        r = RigidStateRecord()
        for n in RIGID_FIELDS:
            a = np.asarray(getattr(self, n), dtype=np.float64).ravel()
            getattr(r, n)[:] = a.tolist()
        r.count, r.entry = int(self.count), int(self.entry)
        return r

    @property
    def frame(self):
        return np.concatenate([self.R.ravel(), self.c])

    @property
    def motion(self):
        return np.concatenate([self.v, self.omega, self.c])

    def same_bits(self, o):
        return self.count == o.count and self.entry == o.entry and all(getattr(self, n).tobytes() == getattr(o, n).tobytes() for n in RIGID_FIELDS)


class GroupMoments(C.Structure):
    """admm_hip_group_moments: a damping group's mass, centre of mass, momentum, angular momentum and inertia about it, angular velocity"""
    _fields_ = [("mass", C.c_double), ("com", C.c_double * 3), ("p", C.c_double * 3), ("l", C.c_double * 3), ("inertia", C.c_double * 6), ("omega", C.c_double * 3),
                ("t_total", C.c_double), ("t_rigid", C.c_double), ("n_nodes", C.c_int64), ("degenerate", C.c_int32), ("pad_", C.c_int32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n in ("mass", "t_total", "t_rigid", "n_nodes", "degenerate")}
        d.update({n: np.array(getattr(self, n)[:]) for n in ("com", "p", "l", "inertia", "omega")})
        return d


class ChamberState(C.Structure):
    """admm_hip_chamber_state: a pressure chamber's volume, area, area vector, pressure, resultant = pressure * area vector"""
    _fields_ = [("volume", C.c_double), ("area", C.c_double), ("area_vector", C.c_double * 3), ("pressure", C.c_double), ("resultant", C.c_double * 3),
                ("n_tris", C.c_int64), ("collapsed", C.c_int64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n in ("volume", "area", "pressure", "n_tris", "collapsed")}
        d.update({n: np.array(getattr(self, n)[:]) for n in ("area_vector", "resultant")})
        return d


def _pressure_law(mode, p, amount, ambient):
    """-> (mode id, params [2]) of a pressure law given by name or id: "constant" takes p, "gas" takes amount and ambient"""
    mid = PRESSURE[mode.upper()] if isinstance(mode, str) else int(mode)
    par = np.array([amount, ambient] if mid == PRESSURE["GAS"] else [p, 0.0], dtype=np.float64)
    return mid, par


class AccelerationRecord(C.Structure):
    _fields_ = [("rho", C.c_double)] + [(n, C.c_int32) for n in ("accepted", "m_used", "extrapolated", "solve_failed")] + \
               [("theta", C.c_double * 8), ("gram", C.c_double * 64), ("rhs", C.c_double * 8)]


class AdmmHipError(RuntimeError):
    pass


_lib = None


def build(force=False, verbose=False):
    return _build.build(force=force, verbose=verbose)


def lib():
    """Loads libadmm_hip.so (rebuilding it when a source is newer: build() checks mtimes).  Raises if it cannot be loaded."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch bundles its own libamdhip64; importing it
        # first makes libadmm_hip.so bind to that copy (same SONAME) so that streams and
        # device pointers can be shared with torch.distributed (bench.py, tests).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        path = os.environ.get("ADMM_HIP_LIB", LIB_PATH)   # experimental variants (tools/ab_local.py)
        if path == LIB_PATH or not os.path.exists(path):
            build()     # no-op when the library is newer than every source (a stale library after an edit is worse than 0.1 s of stat calls)
        L = C.CDLL(path)
        L.admm_hip_last_error.restype = C.c_char_p
        L.admm_hip_last_error.argtypes = [C.c_void_p]
        L.admm_hip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.admm_hip_destroy.argtypes = [C.c_void_p]
        L.admm_hip_destroy.restype = None
        L.admm_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.admm_hip_set_shard_mode.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_set_factor_local.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_debug_node_owner.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.admm_hip_debug_node_supernode.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.admm_hip_local_elements.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]
        L.admm_hip_enable_residuals.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_set_tolerance.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int]
        L.admm_hip_get_residuals.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
        L.admm_hip_energy.argtypes = [C.c_void_p, C.POINTER(EnergyTotals)]
        L.admm_hip_batch_energy.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_batch_energy_dx.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.admm_hip_read_energy_scale.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_energy_query.argtypes = [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, _dp]
        L.admm_hip_batch_gradient.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_batch_gradient_dx.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.admm_hip_batch_stress.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_node_forces.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(ForceInfo)]
        L.admm_hip_gradient_query.argtypes = [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, _dp]
        L.admm_hip_stress_query.argtypes = [C.c_int, C.c_int64, _dp, _dp, _dp, _dp]
        L.admm_hip_enable_objective.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_set_acceleration.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_get_acceleration_log.argtypes = [C.c_void_p, C.POINTER(AccelerationRecord), C.c_int, C.POINTER(C.c_int)]
        L.admm_hip_get_acceleration_default.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.admm_hip_acceleration_query.argtypes = [C.c_int, _dp, _dp, _dp]
        L.admm_hip_batch_reaction.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.admm_hip_node_reactions.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(ReactionInfo)]
        L.admm_hip_get_contacts.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.admm_hip_contact_resultant.argtypes = [C.c_void_p, C.c_double, _dp, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_reaction_query.argtypes = [C.c_int64, _dp, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp, _ip, _dp]
        L.admm_hip_enable_contact_attribution.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_batch_contact_owner.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.admm_hip_get_contact_owners.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.admm_hip_entry_resultants.argtypes = [C.c_void_p, C.c_double, _dp, C.c_int, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_attribution_query.argtypes = [C.c_int64, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp]
        L.admm_hip_add_damping_group.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]
        L.admm_hip_set_damping.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
        L.admm_hip_get_group_moments.argtypes = [C.c_void_p, C.c_int, C.POINTER(GroupMoments)]
        L.admm_hip_damping_query.argtypes = [C.c_int64, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, _dp, C.POINTER(GroupMoments)]
        L.admm_hip_add_pressure_chamber.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, _dp, C.POINTER(C.c_int)]
        L.admm_hip_set_pressure.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.admm_hip_get_chamber_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(ChamberState)]
        L.admm_hip_pressure_query.argtypes = [C.c_int64, _dp, _dp, C.c_int, C.POINTER(C.c_int64), _ip, _ip, _dp, C.c_double, _dp, C.POINTER(ChamberState)]
        L.admm_hip_set_surface_reaction.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.admm_hip_set_surface_reaction_depth.argtypes = [C.c_void_p, C.c_double]
        L.admm_hip_get_surface_reaction.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(SurfaceReactionInfo)]
        L.admm_hip_surface_reaction_query.argtypes = [C.c_int64, _dp, C.c_int64, _dp, _ip, _dp, _dp, C.c_double, _dp]
        L.admm_hip_debug_stable_sort.argtypes = [C.c_void_p, C.c_int64, _ip, C.c_int64, _ip]
        L.admm_hip_add_rigid_body.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, _dp, _dp, C.POINTER(C.c_int)]
        L.admm_hip_set_rigid_depth.argtypes = [C.c_void_p, C.c_double]
        L.admm_hip_get_rigid_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(RigidStateRecord)]
        L.admm_hip_set_rigid_state.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        L.admm_hip_set_rigid_accel.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_get_rigid_body.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp, _dp, _dp, _dp]
        L.admm_hip_rigid_query.argtypes = [C.c_int, C.c_double, _dp, _dp, _dp, _dp, C.POINTER(RigidStateRecord), _dp, _dp, C.c_int64, C.c_double, C.POINTER(RigidStateRecord)]
        L.admm_hip_attach_anchors.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.admm_hip_detach_anchors.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_get_attachment.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp, _dp]
        L.admm_hip_get_attachment_load.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_attachment_query.argtypes = [C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp, C.POINTER(C.c_int64)]
        L.admm_hip_get_objective.argtypes = [C.c_void_p, _dp, _dp, C.c_int, C.POINTER(C.c_int)]
        L.admm_hip_set_timestep.argtypes = [C.c_void_p, C.c_double]
        L.admm_hip_add_nodes.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_int)]
        L.admm_hip_add_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _dp, _dp, C.POINTER(C.c_int)]
        L.admm_hip_add_gravity.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
        L.admm_hip_set_gravity.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
        L.admm_hip_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.admm_hip_add_explicit.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int, _ip, C.POINTER(C.c_int)]
        L.admm_hip_set_collision_shapes.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.admm_hip_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
        L.admm_hip_finalize.argtypes = [C.c_void_p]
        L.admm_hip_set_weights.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_recompute_weights.argtypes = [C.c_void_p]
        L.admm_hip_update_anchors.argtypes = [C.c_void_p, C.c_int, _dp, _ip]
        L.admm_hip_step.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_sync.argtypes = [C.c_void_p]
        for n in ("get_x", "get_v", "debug_rhs"):
            getattr(L, "admm_hip_" + n).argtypes = [C.c_void_p, _dp]
        for n in ("set_x", "set_v", "local_step_only"):
            getattr(L, "admm_hip_" + n).argtypes = [C.c_void_p, _dp]
        L.admm_hip_read_local.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _ip]
        L.admm_hip_write_local.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.admm_hip_read_rest.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip]
        L.admm_hip_solve_only.argtypes = [C.c_void_p, _dp, _dp]
        L.admm_hip_local_step_dx.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_apply_A.argtypes = [C.c_void_p, _dp, _dp]
        L.admm_hip_debug_panel_solve_host.argtypes = [C.c_void_p, _dp, _dp]
        L.admm_hip_debug_math.argtypes = [C.c_void_p, C.c_int, C.c_int64, _dp, _dp]
        L.admm_hip_debug_gemm.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_double, C.c_double, _dp, C.c_int64, _dp, C.c_int64, _dp, C.c_int64]
        L.admm_hip_debug_potrf_inv.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
        L.admm_hip_add_generic_batch.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int64, _ip, _ip, _dp, _dp, C.POINTER(C.c_int)]
        L.admm_hip_set_project_hook.argtypes = [C.c_void_p, PROJECT_FN, C.c_void_p]
        L.admm_hip_rccl_unique_id.argtypes = [C.c_void_p]
        L.admm_hip_rccl_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.admm_hip_set_rccl_comm.argtypes = [C.c_void_p, C.c_void_p]
        L.admm_hip_debug_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.admm_hip_rccl_async_error.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.admm_hip_allreduce_host.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.admm_hip_debug_graph_state.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
        L.admm_hip_pin_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.admm_hip_upload_state.argtypes = [C.c_void_p, _dp, _dp]
        L.admm_hip_download_state.argtypes = [C.c_void_p, _dp, _dp]
        L.admm_hip_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
        L.admm_hip_enable_timing.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_keep_z.argtypes = [C.c_void_p, C.c_int]
        L.admm_hip_get_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
        L.admm_hip_get_timing_previous.argtypes = [C.c_void_p, C.POINTER(Timing)]
        L.admm_hip_mesh_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, _dp, C.c_int, _ip, C.c_char_p, C.c_int]
        L.admm_hip_mesh_destroy.argtypes = [C.c_void_p]
        L.admm_hip_mesh_destroy.restype = None
        L.admm_hip_mesh_query.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, _dp]
        L.admm_hip_mesh_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _dp]
        L.admm_hip_add_collision_mesh.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.admm_hip_mesh_set_vertices.argtypes = [C.c_void_p, C.c_int, _dp, C.c_char_p, C.c_int]
        L.admm_hip_update_collision_mesh.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.admm_hip_add_body_surface.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, C.POINTER(C.c_int)]
        L.admm_hip_set_collision_mesh_owner.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.admm_hip_get_body_surface_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.admm_hip_collision_mesh_copy.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.admm_hip_set_collision_friction.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_friction_query.argtypes = [C.c_int64, _dp, _dp, _dp, _dp, _dp, _ip]
        L.admm_hip_set_collision_motion.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_set_collision_mesh_velocity.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.admm_hip_set_body_surface_friction.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.admm_hip_friction_query_moving.argtypes = [C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _ip]
        L.admm_hip_mesh_velocity_query.argtypes = [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _dp, _ip]
        L.admm_hip_set_collision_frames.argtypes = [C.c_void_p, C.c_int, _dp]
        L.admm_hip_shape_query.argtypes = [C.c_int, _dp, _dp, C.c_int64, _dp, _dp, _ip]
        L.admm_hip_mesh_query_framed.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, _dp, _dp, _dp]
        L.admm_hip_debug_collision_form.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.admm_hip_mesh_create_open.argtypes = [C.POINTER(C.c_void_p), C.c_int, _dp, C.c_int, _ip, C.c_double, C.c_char_p, C.c_int]
        L.admm_hip_mesh_thickness.argtypes = [C.c_void_p, _dp]
        L.admm_hip_mesh_closest.argtypes = [C.c_void_p, C.c_int64, _dp, C.c_double, _dp, _dp, _ip, _ip, _ip]
        L.admm_hip_set_collision_mesh_thickness.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.admm_hip_add_sheet_surface.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, C.c_double, C.POINTER(C.c_int)]
        L.admm_hip_set_sheet_self_collision.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.admm_hip_mesh_query_excluding.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, _dp, _dp, _dp, _dp, _ip]
        L.admm_hip_mesh_velocity_query_excluding.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, _dp, _dp, _dp, _dp, _ip]
        L.admm_hip_set_collision_mesh_side_memory.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.admm_hip_get_collision_sides.argtypes = [C.c_void_p, C.c_int, _ip]
        L.admm_hip_set_collision_sides.argtypes = [C.c_void_p, C.c_int, _ip]
        L.admm_hip_latch_collision_sides.argtypes = [C.c_void_p]
        L.admm_hip_reset_collision_sides.argtypes = [C.c_void_p]
        L.admm_hip_mesh_side_latch.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, C.c_double, _dp, _dp, _ip]
        L.admm_hip_mesh_query_sided.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, C.c_double, _dp, _dp, _dp, _dp, _ip, _ip]
        L.admm_hip_mesh_boundary_table.argtypes = [C.c_void_p, _ip, _ip]
        L.admm_hip_mesh_feature_normal.argtypes = [C.c_void_p, C.c_int64, _ip, _ip, _dp]
        L.admm_hip_set_body_self_collision.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
        L.admm_hip_mesh_query_self.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, _dp, C.c_double, C.c_double, C.c_double, _dp, _dp, _ip, _ip]
        L.admm_hip_mesh_velocity_query_self.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_ip) if a is not None else None


class Mesh:
    """A closed triangle mesh prepared for collision queries (admm_hip_mesh_create): validated, pseudo-normals and BVH built.
    verts [nv][3] float64, tris [nt][3] int32, counter-clockwise seen from outside.  Invalid input raises AdmmHipError.
    half_thickness given: an open surface (admm_hip_mesh_create_open; boundary edges allowed, a closed input too), which collides as
    a shell of that half thickness: query then returns the point after the shell rule and sdist = r - d (-inf beyond r)."""

    def __init__(self, verts, tris=None, half_thickness=None):
        self.L = lib()
        if isinstance(verts, C.c_void_p):      # an admm_hip_mesh handle this object takes over (System.collision_mesh)
            self.h = verts
            return
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        if half_thickness is not None:
            rc = self.L.admm_hip_mesh_create_open(C.byref(h), v.shape[0], _d(v), t.shape[0], _i(t), float(half_thickness), err, len(err))
            if rc != 0:
                raise AdmmHipError("admm_hip_mesh_create_open error %d: %s" % (rc, err.value.decode()))
            self.h = h
            return
        rc = self.L.admm_hip_mesh_create(C.byref(h), v.shape[0], _d(v), t.shape[0], _i(t), err, len(err))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_create error %d: %s" % (rc, err.value.decode()))
        self.h = h

    @property
    def thickness(self):
        """the half thickness of an open mesh (a shell); 0.0 for a closed mesh"""
        r = np.zeros(1)
        self.L.admm_hip_mesh_thickness(self.h, _d(r))
        return float(r[0])

    def closest(self, q, r2=None):
        """the closest-point search as it runs (admm_hip_mesh_closest) for q [n][3] relative to the mesh: the unbounded one, or with r2
        the one bounded by it -> dict(c [n][3], d2 [n], slot [n], reg [n], tri [n]); slot -1: no triangle nearer than sqrt(r2)"""
        p = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
        n = p.shape[0]
        c = np.empty((n, 3)); d2 = np.empty(n)
        slot = np.empty(n, dtype=np.int32); reg = np.empty(n, dtype=np.int32); tri = np.empty(n, dtype=np.int32)
        rc = self.L.admm_hip_mesh_closest(self.h, n, _d(p), -1.0 if r2 is None else float(r2), _d(c), _d(d2), _i(slot), _i(reg), _i(tri))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_closest error %d" % rc)
        return dict(c=c, d2=d2, slot=slot, reg=reg, tri=tri)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.admm_hip_mesh_destroy(self.h)
            self.h = None

    def query(self, pts, t=(0.0, 0.0, 0.0), frame=None):
        """-> (proj [n][3], sdist [n]) for the instance translated by t: proj = t + the closest point, sdist > 0 inside (host evaluation);
        frame [12] = (R row-major, pivot): the instance rotated by R about the pivot (admm_hip_mesh_query_framed), proj in world coordinates"""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        proj = np.empty_like(p); sd = np.empty(p.shape[0])
        if frame is not None:
            f = frame_array(frame)
            rc = self.L.admm_hip_mesh_query_framed(self.h, _d(tt), _d(f), p.shape[0], _d(p), _d(proj), _d(sd))
            if rc != 0:
                raise AdmmHipError("admm_hip_mesh_query_framed error %d" % rc)
            return proj, sd
        rc = self.L.admm_hip_mesh_query(self.h, _d(tt), p.shape[0], _d(p), _d(proj), _d(sd))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_query error %d" % rc)
        return proj, sd

    def query_excluding(self, pts, skip_vertex, t=(0.0, 0.0, 0.0), frame=None):
        """the shell rule of an open mesh with a per-point excluded vertex (admm_hip_mesh_query_excluding; self-collision of a sheet): the
        bounded search of point i ignores every triangle that has vertex skip_vertex[i] as a corner (-1: none, the bits of query) ->
        (proj [n][3], sdist [n], tri [n]: the winning original triangle, -1: none nearer than the half thickness).  A closed mesh or an
        id outside [-1, nv) raises AdmmHipError."""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        sk = np.ascontiguousarray(np.broadcast_to(np.asarray(skip_vertex, dtype=np.int32), (p.shape[0],)))
        tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        f = None if frame is None else frame_array(frame)
        proj = np.empty_like(p); sd = np.empty(p.shape[0]); tri = np.empty(p.shape[0], np.int32)
        rc = self.L.admm_hip_mesh_query_excluding(self.h, p.shape[0], _d(p), _i(sk), _d(tt), _d(f), _d(proj), _d(sd), _i(tri))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_query_excluding error %d" % rc)
        return proj, sd, tri

    def velocity_query_excluding(self, pts, skip_vertex, vel, t=(0.0, 0.0, 0.0)):
        """mesh_velocity_query at the hit of query_excluding's search (admm_hip_mesh_velocity_query_excluding) -> (out, weights,
        corner_ids); zeros and ids -1 where no triangle outside the excluded 1-ring is nearer than the half thickness"""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        sk = np.ascontiguousarray(np.broadcast_to(np.asarray(skip_vertex, dtype=np.int32), (p.shape[0],)))
        tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
        out = np.empty_like(p); wts = np.empty_like(p); ids = np.empty(p.shape, np.int32)
        rc = self.L.admm_hip_mesh_velocity_query_excluding(self.h, p.shape[0], _d(p), _i(sk), _d(tt), _d(v), _d(out), _d(wts), _i(ids))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_velocity_query_excluding error %d" % rc)
        return out, wts, ids

    def side_latch(self, pts, prev, reach, t=(0.0, 0.0, 0.0), frame=None):
        """the latch of side memory (admm_hip_mesh_side_latch) on an open mesh with the given reach: the new side [n] int32 of every point
        from its previous one (prev: [n] in {-1, 0, 1}, a scalar, or None for all 0), for the instance translated by t under a frame"""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        pv = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if prev is None else prev, dtype=np.int32), (p.shape[0],)))
        tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        f = None if frame is None else frame_array(frame)
        out = np.empty(p.shape[0], np.int32)
        rc = self.L.admm_hip_mesh_side_latch(self.h, p.shape[0], _d(p), _i(pv), float(reach), _d(tt), _d(f), _i(out))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_side_latch error %d" % rc)
        return out

    def query_sided(self, pts, side, reach, t=(0.0, 0.0, 0.0), frame=None):
        """the projection of side memory (admm_hip_mesh_query_sided) -> (proj [n][3], sdist [n], tri [n], crossed [n]): a point with side 0
        runs the shell rule (the bits of query), one with side +-1 stays on that side of the surface within the reach; sdist = r - d for
        an unsigned push, r + d for a crossed one, -inf for none"""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        sd_ = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if side is None else side, dtype=np.int32), (p.shape[0],)))
        tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        f = None if frame is None else frame_array(frame)
        proj = np.empty_like(p); sd = np.empty(p.shape[0]); tri = np.empty(p.shape[0], np.int32); cr = np.empty(p.shape[0], np.int32)
        rc = self.L.admm_hip_mesh_query_sided(self.h, p.shape[0], _d(p), _i(sd_), float(reach), _d(tt), _d(f), _d(proj), _d(sd), _i(tri), _i(cr))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_query_sided error %d" % rc)
        return proj, sd, tri, cr

    def query_self(self, pts, vertex_id, rest_verts, r, reach, rest_radius):
        """self-collision of a closed body surface (admm_hip_mesh_query_self) -> (proj [n][3], sdist [n], tri [n], crossed [n]): point i
        is vertex vertex_id[i] of this closed mesh (-1: an interior node, left alone) and meets the triangles within the reach that are
        not within rest_radius of that vertex in the rest shape rest_verts [nv][3]: pushed to distance r when nearer outside, mirrored
        to distance r outside when it has crossed the skin; sdist = r - d for a hit on the outside (> 0: pushed), r + d for a crossed
        point, -inf for no hit; tri: the winning triangle of a hit, -1 for none"""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        vid = np.ascontiguousarray(np.broadcast_to(np.asarray(vertex_id, dtype=np.int32), (p.shape[0],)))
        X = np.ascontiguousarray(rest_verts, dtype=np.float64).reshape(-1, 3)
        proj = np.empty_like(p); sd = np.empty(p.shape[0]); tri = np.empty(p.shape[0], np.int32); cr = np.empty(p.shape[0], np.int32)
        rc = self.L.admm_hip_mesh_query_self(self.h, p.shape[0], _d(p), _i(vid), _d(X), float(r), float(reach), float(rest_radius), _d(proj), _d(sd), _i(tri), _i(cr))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_query_self error %d" % rc)
        return proj, sd, tri, cr

    def velocity_query_self(self, pts, vertex_id, rest_verts, reach, rest_radius, vel):
        """mesh_velocity_query at the hit of query_self's search (admm_hip_mesh_velocity_query_self) -> (out, weights, corner_ids);
        a point without a hit within the reach gets zeros and ids -1"""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        vid = np.ascontiguousarray(np.broadcast_to(np.asarray(vertex_id, dtype=np.int32), (p.shape[0],)))
        X = np.ascontiguousarray(rest_verts, dtype=np.float64).reshape(-1, 3)
        v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
        if v.shape != X.shape:
            raise AdmmHipError("velocity_query_self: %d velocities given, the rest shape has %d vertices" % (v.shape[0], X.shape[0]))
        out = np.empty_like(p); wts = np.empty_like(p); ids = np.empty((p.shape[0], 3), np.int32)
        rc = self.L.admm_hip_mesh_velocity_query_self(self.h, p.shape[0], _d(p), _i(vid), _d(X), float(reach), float(rest_radius), _d(v), _d(out), _d(wts), _i(ids))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_velocity_query_self error %d" % rc)
        return out, wts, ids

    def boundary_table(self):
        """-> (bits [nt], orig [nt]) per leaf slot (admm_hip_mesh_boundary_table): bit reg (1..6) set where that feature of the slot's
        triangle is a boundary edge or a vertex incident to one; orig: the slot's original triangle"""
        nt = self.info()["n_tris"]
        bits = np.empty(nt, np.int32); orig = np.empty(nt, np.int32)
        self.L.admm_hip_mesh_boundary_table(self.h, _i(bits), _i(orig))
        return bits, orig

    def feature_normal(self, slot, reg):
        """the stored pseudo-normal [n][3] of the features (slot, reg) that closest returns (admm_hip_mesh_feature_normal)"""
        sl = np.ascontiguousarray(slot, dtype=np.int32).ravel(); rg = np.ascontiguousarray(reg, dtype=np.int32).ravel()
        out = np.empty((sl.size, 3))
        rc = self.L.admm_hip_mesh_feature_normal(self.h, sl.size, _i(sl), _i(rg), _d(out))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_feature_normal error %d" % rc)
        return out

    def set_vertices(self, verts):
        """new vertex positions [nv][3] for the same topology (admm_hip_mesh_set_vertices): pseudo-normals recomputed, BVH boxes refit.
        A refused update raises AdmmHipError and leaves the mesh as it was."""
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        err = C.create_string_buffer(512)
        rc = self.L.admm_hip_mesh_set_vertices(self.h, v.shape[0], _d(v), err, len(err))
        if rc != 0:
            raise AdmmHipError("admm_hip_mesh_set_vertices error %d: %s" % (rc, err.value.decode()))

    def info(self):
        nt, nn, dep = C.c_int(), C.c_int(), C.c_int()
        box = np.zeros(6)
        self.L.admm_hip_mesh_info(self.h, C.byref(nt), C.byref(nn), C.byref(dep), _d(box))
        return dict(n_tris=nt.value, n_nodes=nn.value, depth=dep.value, lo=box[:3].copy(), hi=box[3:].copy())


def mesh_query(verts, tris, pts, t=(0.0, 0.0, 0.0), frame=None):
    """closest points and signed distances of pts to the closed mesh (verts, tris; a Mesh for verts: tris ignored) translated by t and, with
    frame [12], rotated about its pivot -> (proj, sdist), sdist > 0 inside"""
    return (verts if isinstance(verts, Mesh) else Mesh(verts, tris)).query(pts, t, frame)


def frame_array(frame):
    """one frame as the ABI takes it, 12 doubles (R row-major, pivot), from that or from a pair (R [3][3], pivot [3])"""
    if isinstance(frame, (tuple, list)) and len(frame) == 2:
        frame = np.concatenate([np.asarray(frame[0], dtype=np.float64).reshape(9), np.asarray(frame[1], dtype=np.float64).reshape(3)])
    return np.ascontiguousarray(frame, dtype=np.float64).reshape(12)


def shape_query(type_, params, pts, frame=None):
    """one analytic entry of a shape list (floor, sphere, cylinder, box) with its frame on the host (admm_hip_shape_query) ->
    (out [n][3]: the points after the entry, moved [n] bool); the device's kernels give the same bits"""
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    par = np.ascontiguousarray(params, dtype=np.float64).reshape(4)
    f = None if frame is None else frame_array(frame)
    out = np.empty_like(p); moved = np.empty(p.shape[0], np.int32)
    rc = lib().admm_hip_shape_query(int(type_), _d(par), _d(f), p.shape[0], _d(p), _d(out), _i(moved))
    if rc != 0:
        raise AdmmHipError("admm_hip_shape_query error %d" % rc)
    return out, moved.astype(bool)


def friction_query(p, p_out, x0, mu):
    """the contact friction rule on the host (admm_hip_friction_query): p, p_out (where a shape put p), x0 (the frame-start positions)
    [n][3], mu [n] or a scalar -> (result [n][3], mode [n]: 0 none, 1 stick, 2 slip); the device's kernel gives the same bits"""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    po = np.ascontiguousarray(p_out, dtype=np.float64).reshape(-1, 3)
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, 3)
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (p.shape[0],)))
    assert po.shape == p.shape and x0.shape == p.shape
    res = np.empty_like(p); mode = np.empty(p.shape[0], np.int32)
    rc = lib().admm_hip_friction_query(p.shape[0], _d(p), _d(po), _d(x0), _d(m), _d(res), _i(mode))
    if rc != 0:
        raise AdmmHipError("admm_hip_friction_query error %d" % rc)
    return res, mode


def friction_query_moving(p, p_out, x0, w, mu):
    """the friction rule against a moving obstacle on the host (admm_hip_friction_query_moving): as friction_query, with w [n][3] the
    displacement of the obstacle's surface over the frame at each contact; w = 0 gives the bits of friction_query"""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    po = np.ascontiguousarray(p_out, dtype=np.float64).reshape(-1, 3)
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, 3)
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), p.shape))
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (p.shape[0],)))
    assert po.shape == p.shape and x0.shape == p.shape
    res = np.empty_like(p); mode = np.empty(p.shape[0], np.int32)
    rc = lib().admm_hip_friction_query_moving(p.shape[0], _d(p), _d(po), _d(x0), _d(w), _d(m), _d(res), _i(mode))
    if rc != 0:
        raise AdmmHipError("admm_hip_friction_query_moving error %d" % rc)
    return res, mode


def energy_query(kind, dx, params, rest, scale):
    """the elements' energies on the host (admm_hip_energy_query; csrc/energy.hpp, the device's bits; needs no GPU): dx [n][rows] = D_i x,
    params [n][KIND_PARAMS] (or one row for all), rest [n][12] as read_rest lays it out (or None: zeros), scale [n] (or a scalar)
    -> energy [n]; +inf where the kind's energy is infinite"""
    kind = KIND[kind] if isinstance(kind, str) else int(kind)
    if not 0 <= kind < len(KIND_ROWS):
        rc = lib().admm_hip_energy_query(kind, 0, None, None, None, None, None)
        raise AdmmHipError("admm_hip_energy_query error %d" % rc)
    dx = np.ascontiguousarray(dx, dtype=np.float64).reshape(-1, KIND_ROWS[kind])
    n = dx.shape[0]
    par = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64).reshape(-1, KIND_PARAMS[kind]), (n, KIND_PARAMS[kind])))
    rs = np.zeros((n, 12)) if rest is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rest, dtype=np.float64).reshape(-1, 12), (n, 12)))
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,)))
    out = np.zeros(n)
    rc = lib().admm_hip_energy_query(kind, n, _d(dx), _d(par), _d(rs), _d(sc), _d(out))
    if rc:
        raise AdmmHipError("admm_hip_energy_query error %d" % rc)
    return out


def gradient_query(kind, dx, params, rest, scale):
    """the elements' gradients g = dE/dd on the host (admm_hip_gradient_query; csrc/gradient.hpp, the device's bits; needs no GPU), with
    the arguments of energy_query -> g [n][rows]; NaN rows where the kind's energy is infinite.  TET_VOLUME and TRI_AREA return the
    projective force s (d - p), which is not the derivative of their stored energy (include/admm_hip.h)"""
    kind = KIND[kind] if isinstance(kind, str) else int(kind)
    if not 0 <= kind < len(KIND_ROWS):
        rc = lib().admm_hip_gradient_query(kind, 0, None, None, None, None, None)
        raise AdmmHipError("admm_hip_gradient_query error %d" % rc)
    dx = np.ascontiguousarray(dx, dtype=np.float64).reshape(-1, KIND_ROWS[kind])
    n = dx.shape[0]
    par = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64).reshape(-1, KIND_PARAMS[kind]), (n, KIND_PARAMS[kind])))
    rs = np.zeros((n, 12)) if rest is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rest, dtype=np.float64).reshape(-1, 12), (n, 12)))
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,)))
    out = np.zeros((n, KIND_ROWS[kind]))
    rc = lib().admm_hip_gradient_query(kind, n, _d(dx), _d(par), _d(rs), _d(sc), _d(out))
    if rc:
        raise AdmmHipError("admm_hip_gradient_query error %d" % rc)
    return out


def acceleration_query(gram, rhs):
    """the small solve of Anderson acceleration on the host (admm_hip_acceleration_query; csrc/anderson.hpp, the device's bits; needs no
    GPU): gram [m_k][m_k] = dF^T W^2 dF before regularisation (its lower triangle is read), rhs [m_k] -> theta [m_k], the solution of
    (gram + 1e-12 tr(gram) / m_k I) theta = rhs; zeros where a Cholesky pivot is not positive.  1 <= m_k <= 8."""
    A = np.ascontiguousarray(gram, dtype=np.float64)
    b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
    mk = b.size
    if A.ndim != 2 or A.shape != (mk, mk) or not 1 <= mk <= 8:
        rc = lib().admm_hip_acceleration_query(0, None, None, None)
        raise AdmmHipError("admm_hip_acceleration_query error %d" % rc)
    th = np.zeros(mk)
    rc = lib().admm_hip_acceleration_query(mk, _d(A), _d(b), _d(th))
    if rc:
        raise AdmmHipError("admm_hip_acceleration_query error %d" % rc)
    return th


def reaction_query(w2, u, z, x, depth_min=1e-10, pivot=(0.0, 0.0, 0.0)):
    """the reactions of one-node constraints on the host (admm_hip_reaction_query; csrc/reaction.hpp, the device's bits; needs no GPU):
    w2 [n] (or a scalar): weight^2, u, z, x [n][3] -> dict(f [n][3] = w2 ((z - u) - x), depth [n] = |u|, flag [n] = depth > depth_min,
    force [3], torque [3]: the resultant of the flagged elements about `pivot`, summed in the order csrc/reaction.hpp states)"""
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 3)
    n = u.shape[0]
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 3)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    assert z.shape == u.shape and x.shape == u.shape
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(w2, dtype=np.float64), (n,)))
    pv = np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
    f = np.zeros((n, 3)); depth = np.zeros(n); flag = np.zeros(n, np.int32); r6 = np.zeros(6)
    rc = lib().admm_hip_reaction_query(n, _d(w), _d(u), _d(z), _d(x), float(depth_min), _d(pv), _d(f), _d(depth), _i(flag), _d(r6))
    if rc:
        raise AdmmHipError("admm_hip_reaction_query error %d" % rc)
    return dict(f=f, depth=depth, flag=flag.astype(bool), force=r6[:3].copy(), torque=r6[3:].copy())


def attribution_query(before=None, after=None, f=None, normal=None):
    """the contact attribution rule on the host (admm_hip_attribution_query; csrc/attribution.hpp, the device's bits; needs no GPU):
    before, after [n][3]: a candidate before an entry's rule and behind it (before friction), f [n][3]: reactions (default: zeros) ->
    dict(moved [n]: a coordinate's bits differ, normal [n][3]: (after - before) / its length, 0 where not moved, fn [n], ft [n][3]: f's
    part along the normal and the rest).  normal [n][3] given: the split is about these normals, and before / after may be left out."""
    first = before if before is not None else normal
    n = np.ascontiguousarray(first, dtype=np.float64).reshape(-1, 3).shape[0]
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(n, 3)
    b, a, nin = arr(before), arr(after), arr(normal)
    ff = np.zeros((n, 3)) if f is None else arr(f)
    moved = np.zeros(n, np.int32); nr = np.zeros((n, 3)); fn = np.zeros(n); ft = np.zeros((n, 3))
    ptr = lambda v: None if v is None else _d(v)
    rc = lib().admm_hip_attribution_query(n, ptr(b), ptr(a), _d(ff), ptr(nin), _i(moved), _d(nr), _d(fn), _d(ft))
    if rc:
        raise AdmmHipError("admm_hip_attribution_query error %d" % rc)
    return dict(moved=moved.astype(bool), normal=nr, fn=fn, ft=ft)


def damping_query(m, x, v, dt, drag, internal):
    """the velocity filter of one damping group on the host (admm_hip_damping_query; csrc/damping.hpp, the device's bits; needs no GPU):
    m [n] (or a scalar): the nodes' masses, x, v [n][3], dt, the rates drag and internal in 1/s -> (v_out [n][3], moments: the dict of
    System.group_moments for the input state)"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    assert v.shape == x.shape
    mm = np.ascontiguousarray(np.broadcast_to(np.asarray(m, dtype=np.float64), (n,)))
    out = np.zeros((n, 3)); rec = GroupMoments()
    rc = lib().admm_hip_damping_query(n, _d(mm), _d(x), _d(v), float(dt), float(drag), float(internal), _d(out), C.byref(rec))
    if rc:
        raise AdmmHipError("admm_hip_damping_query error %d" % rc)
    return out, rec.as_dict()


def pressure_query(x, m, chambers, dt):
    """the pressure chambers' load on the host (admm_hip_pressure_query; csrc/pressure.hpp, the device's bits; needs no GPU): x [nv][3],
    m [nv] (or a scalar): the nodes' masses, chambers: one dict or a list of dicts(tris=[nt][3], mode="constant" | "gas", p=, amount=,
    ambient=) as System.add_pressure_chamber takes them, dt -> (dv [nv][3], the list of the chambers' records as System.chamber_state
    returns them; `collapsed` is 1 where this evaluation found a gas chamber's volume not positive)"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    nv = x.shape[0]
    mm = np.ascontiguousarray(np.broadcast_to(np.asarray(m, dtype=np.float64), (nv,)))
    if isinstance(chambers, dict):
        chambers = [chambers]
    tl = [np.ascontiguousarray(c["tris"], dtype=np.int32).reshape(-1, 3) for c in chambers]
    laws = [_pressure_law(c.get("mode", "constant"), c.get("p", 0.0), c.get("amount", 0.0), c.get("ambient", 0.0)) for c in chambers]
    ptr = np.concatenate([[0], np.cumsum([len(t) for t in tl])]).astype(np.int64)
    tris = np.ascontiguousarray(np.concatenate(tl) if tl else np.zeros((0, 3), np.int32))
    mode = np.array([l[0] for l in laws], dtype=np.int32)
    par = np.ascontiguousarray(np.array([l[1] for l in laws], dtype=np.float64).reshape(-1, 2))
    dv = np.zeros((nv, 3)); recs = (ChamberState * max(len(tl), 1))()
    rc = lib().admm_hip_pressure_query(nv, _d(x), _d(mm), len(tl), ptr.ctypes.data_as(C.POINTER(C.c_int64)), _i(tris), _i(mode), _d(par), float(dt), _d(dv), recs)
    if rc:
        raise AdmmHipError("admm_hip_pressure_query error %d" % rc)
    return dv, [recs[c].as_dict() for c in range(len(tl))]


def surface_reaction_query(m3, f, corner, weight, share, dt):
    """two-way contact's shares and ordered sums on the host (admm_hip_surface_reaction_query; csrc/surface_reaction.hpp, the device's
    bits; needs no GPU): m3 [n_nodes][3] the nodes' mass per component (or [n_nodes]: one mass per node), and per contact f [K][3],
    corner [K][3] (node ids), weight [K][3], share [K] (or a scalar), dt -> dv [n_nodes][3]: v <- v - dv.  A row with share 0 adds
    nothing."""
    mm = np.asarray(m3, dtype=np.float64)
    if mm.ndim == 1:
        mm = np.repeat(mm[:, None], 3, axis=1)
    mm = np.ascontiguousarray(mm.reshape(-1, 3))
    n = mm.shape[0]
    f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 3)
    K = f.shape[0]
    cn = np.ascontiguousarray(corner, dtype=np.int32).reshape(-1, 3)
    w = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1, 3)
    sh = np.ascontiguousarray(np.broadcast_to(np.asarray(share, dtype=np.float64), (K,)))
    assert cn.shape[0] == K and w.shape[0] == K
    dv = np.zeros((n, 3))
    rc = lib().admm_hip_surface_reaction_query(n, _d(mm), K, _d(f), _i(cn), _d(w), _d(sh), float(dt), _d(dv))
    if rc:
        raise AdmmHipError("admm_hip_surface_reaction_query error %d" % rc)
    return dv


def rigid_query(state, row, dt, count=0, body=None):
    """one frame of a rigid body on the host (admm_hip_rigid_query; csrc/rigid.hpp, the device's bits; needs no GPU): state a
    RigidState, row [6] = the body's {sum f, sum (point - c) x f} of entry_resultants(pivot = state.c), dt, count the row's number of
    contacts; body (default state.body): dict(type, mass, inertia [6] = xx xy xz yy yz zz, accel [3], c0 [3], par0 [4]) -> RigidState"""
    K = state.body if body is None else body
    a = {n: np.ascontiguousarray(K[n], dtype=np.float64) for n in ("inertia", "accel", "c0", "par0")}
    assert a["inertia"].size == 6 and a["accel"].size == 3 and a["c0"].size == 3 and a["par0"].size == 4
    r = np.ascontiguousarray(row, dtype=np.float64).reshape(6)
    fe, te = r[:3].copy(), r[3:].copy()
    rin, out = state.record(), RigidStateRecord()
    ty = SHAPE[K["type"]] if isinstance(K["type"], str) else int(K["type"])
    rc = lib().admm_hip_rigid_query(ty, float(K["mass"]), _d(a["inertia"]), _d(a["accel"]), _d(a["c0"]), _d(a["par0"]), C.byref(rin), _d(fe), _d(te), int(count), float(dt), C.byref(out))
    if rc:
        raise AdmmHipError("admm_hip_rigid_query error %d" % rc)
    return RigidState(out, K)


def attachment_query(c=None, R=None, local=None, f=None, point=None, active=None, pivot=None):
    """rigid attachments on the host (admm_hip_attachment_query; csrc/attach.hpp, the device's bits; needs no GPU).  Target half, when
    `local` [n][3] is given: targets [n][3] = c + R local from a body's c [3] and R [3][3].  Sum half, when `f` [n][3] is given: the row
    {sum f, sum (point - pivot) x f} over the elements in the device's order from f and point [n][3] (batch_reaction's f, read_local's
    z), active [n] (None: all active; a released element adds zeros) and pivot [3].  -> dict with targets and / or row [6], n_active"""
    out = {}
    if local is not None:
        loc = np.ascontiguousarray(local, dtype=np.float64).reshape(-1, 3)
        cc = np.ascontiguousarray(c, dtype=np.float64).reshape(3); rr = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        tg = np.zeros_like(loc)
        rc = lib().admm_hip_attachment_query(len(loc), _d(cc), _d(rr), _d(loc), _d(tg), None, None, None, None, None, None)
        if rc:
            raise AdmmHipError("admm_hip_attachment_query error %d" % rc)
        out["targets"] = tg
    if f is not None:
        ff = np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 3); pt = np.ascontiguousarray(point, dtype=np.float64).reshape(-1, 3)
        assert ff.shape == pt.shape
        ac = None if active is None else np.ascontiguousarray(active, dtype=np.int32).reshape(len(ff))
        pv = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
        row = np.zeros(6); na = C.c_int64(0)
        rc = lib().admm_hip_attachment_query(len(ff), None, None, None, None, _d(ff), _d(pt), _i(ac), _d(pv), _d(row), C.byref(na))
        if rc:
            raise AdmmHipError("admm_hip_attachment_query error %d" % rc)
        out["row"] = row; out["n_active"] = int(na.value)
    return out


def stress_query(kind, dx, params, volume):
    """the tets' Cauchy stress on the host (admm_hip_stress_query; the device's bits; needs no GPU): dx [n][9], params [n][KIND_PARAMS] (or
    one row for all), volume [n] (or a scalar): the rest volumes -> stress [n][7]: xx, yy, zz, xy, xz, yz, von Mises; NaN where J <= 0"""
    kind = KIND[kind] if isinstance(kind, str) else int(kind)
    if kind not in (KIND["TET_LINEAR"], KIND["TET_VOLUME"], KIND["TET_NH"], KIND["TET_STVK"]):
        rc = lib().admm_hip_stress_query(kind, 0, None, None, None, None)
        raise AdmmHipError("admm_hip_stress_query error %d" % rc)
    dx = np.ascontiguousarray(dx, dtype=np.float64).reshape(-1, 9)
    n = dx.shape[0]
    par = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64).reshape(-1, KIND_PARAMS[kind]), (n, KIND_PARAMS[kind])))
    vol = np.ascontiguousarray(np.broadcast_to(np.asarray(volume, dtype=np.float64), (n,)))
    out = np.zeros((n, 7))
    rc = lib().admm_hip_stress_query(kind, n, _d(dx), _d(par), _d(vol), _d(out))
    if rc:
        raise AdmmHipError("admm_hip_stress_query error %d" % rc)
    return out


def mesh_velocity_query(verts, tris, pts, vel, t=(0.0, 0.0, 0.0)):
    """the vertex field vel [nv][3] of the closed mesh (verts, tris; a Mesh for verts: tris ignored) translated by t, interpolated at the
    closest point to each of pts (admm_hip_mesh_velocity_query) -> (out [n][3], weights [n][3], corner_ids [n][3]): the barycentric
    weights of the closest point on its triangle and that triangle's vertex ids; the moving friction kernel gives the same bits"""
    m = verts if isinstance(verts, Mesh) else Mesh(verts, tris)
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(p); wts = np.empty_like(p); ids = np.empty(p.shape, np.int32)
    rc = lib().admm_hip_mesh_velocity_query(m.h, p.shape[0], _d(p), _d(tt), _d(v), _d(out), _d(wts), _i(ids))
    if rc != 0:
        raise AdmmHipError("admm_hip_mesh_velocity_query error %d" % rc)
    return out, wts, ids


class System:
    """Python face of the C ABI with the reference's System vocabulary.

    device_id < 0 gives a host-only context (assembly + factorization only;
    every device call raises) -- used by the CPU test-suite."""

    def __init__(self, device_id=0, stream=None):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.admm_hip_create(C.byref(h), int(device_id))
        if rc != 0:
            raise AdmmHipError("admm_hip_create(device %d) failed with code %d: no usable MI355X/HIP device "
                               "(this package has no CPU fallback)" % (device_id, rc))
        self.h = h
        self.batches = []  # (kind, n)
        self.n_nodes = 0
        self._cb = None
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.admm_hip_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise AdmmHipError("admm_hip error %d: %s" % (rc, self.L.admm_hip_last_error(self.h).decode()))

    def set_stream(self, stream):
        """run on the caller's hipStream_t from now on (admm_hip_set_stream; e.g. torch.cuda.current_stream().cuda_stream), None: on a
        stream of the library's own again.  The caller keeps its stream: the library never destroys it."""
        self._chk(self.L.admm_hip_set_stream(self.h, C.c_void_p(stream) if stream else None))

    # ---- setup (System.hpp:36-63) ----
    def set_timestep(self, dt):
        self._chk(self.L.admm_hip_set_timestep(self.h, float(dt)))

    def add_nodes(self, x, m):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        m = np.ascontiguousarray(m, dtype=np.float64).ravel()
        assert x.size == m.size and x.size % 3 == 0
        tot = C.c_int()
        self._chk(self.L.admm_hip_add_nodes(self.h, x.size // 3, _d(x), _d(m), C.byref(tot)))
        self.n_nodes = tot.value
        return tot.value

    def add_forces(self, kind, idx, params, targets=None):
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, KIND_NODES[kind])
        n = idx.shape[0]
        params = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64), (n, KIND_PARAMS[kind])))
        tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.float64).reshape(n, 3)
        b = C.c_int()
        self._chk(self.L.admm_hip_add_batch(self.h, kind, n, _i(idx), _d(params), _d(tg), C.byref(b)))
        self.batches.append((kind, n))
        return b.value

    def add_generic(self, elem_row_ptr, trip_row, trip_col, trip_val, row_weight):
        """A run of user-defined forces (admm_hip_add_generic_batch): selector rows as triplets (row relative to the batch,
        col = 3 * node + component), one weight per row; project() is the hook installed with set_project_hook."""
        erp = np.ascontiguousarray(elem_row_ptr, dtype=np.int32)
        tr = np.ascontiguousarray(trip_row, dtype=np.int32); tc = np.ascontiguousarray(trip_col, dtype=np.int32)
        tv = np.ascontiguousarray(trip_val, dtype=np.float64); rw = np.ascontiguousarray(row_weight, dtype=np.float64)
        assert tr.size == tc.size == tv.size and rw.size == erp[-1]
        b = C.c_int()
        self._chk(self.L.admm_hip_add_generic_batch(self.h, erp.size - 1, _i(erp), tr.size, _i(tr), _i(tc), _d(tv), _d(rw), C.byref(b)))
        self.batches.append((KIND_GENERIC, erp.size - 1))
        self._generic_rows = getattr(self, "_generic_rows", {})
        self._generic_rows[b.value] = np.diff(erp)
        return b.value

    def set_project_hook(self, pyfunc):
        """pyfunc(dt, Dx, u, z): numpy views over ALL generic rows; update u and z in place (Force::project, System.cpp:57-58)."""
        def tramp(user, dt, n_rows, dx, u, z):
            try:
                n = int(n_rows)
                pyfunc(float(dt), np.ctypeslib.as_array(dx, shape=(n,)), np.ctypeslib.as_array(u, shape=(n,)), np.ctypeslib.as_array(z, shape=(n,)))
                return 0
            except Exception as e:  # never let an exception cross the C boundary
                print("project hook raised:", e)
                return 1
        self._pcb = PROJECT_FN(tramp)
        self._chk(self.L.admm_hip_set_project_hook(self.h, self._pcb, None))

    # ---- RCCL inside the library (admm_hip.h "RCCL inside the library") ----
    def rccl_unique_id(self):
        buf = np.zeros(128, np.uint8)
        rc = self.L.admm_hip_rccl_unique_id(buf.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise AdmmHipError("admm_hip_rccl_unique_id failed (%d)" % rc)
        return buf

    def rccl_init(self, uid, rank, world):
        uid = np.ascontiguousarray(uid, dtype=np.uint8)
        assert uid.size == 128
        self._chk(self.L.admm_hip_rccl_init(self.h, uid.ctypes.data_as(C.c_void_p), int(rank), int(world)))

    def set_rccl_comm(self, comm_ptr):
        self._chk(self.L.admm_hip_set_rccl_comm(self.h, C.c_void_p(comm_ptr) if comm_ptr else None))

    def debug_allreduce(self, dev_ptr, count):
        self._chk(self.L.admm_hip_debug_allreduce(self.h, C.c_void_p(dev_ptr), int(count)))

    def rccl_async_error(self):
        """ncclCommGetAsyncError of the installed communicator: 0 while healthy (raises with RCCL's text otherwise)"""
        r = C.c_int(0)
        self._chk(self.L.admm_hip_rccl_async_error(self.h, C.byref(r)))
        return r.value

    def allreduce_host(self, vec):
        """a short host vector summed in place across the ranks through the installed transport (no-op at world 1)"""
        assert vec.dtype == np.float64 and vec.flags.c_contiguous
        self._chk(self.L.admm_hip_allreduce_host(self.h, _d(vec), vec.size))
        return vec

    def graph_state(self):
        a = C.c_int(0); b = C.c_int(0); n = C.c_int64(0)
        self._chk(self.L.admm_hip_debug_graph_state(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return dict(iter_graph=bool(a.value), frame_graph_iters=b.value, graph_launches=n.value)

    # ---- the class API's frame boundary (host/admm/System.hpp step()) ----
    def pin_host(self, arr, on=True):
        self._chk(self.L.admm_hip_pin_host(self.h, C.c_void_p(arr.ctypes.data), arr.nbytes, 1 if on else 0))

    def upload_state(self, x=None, v=None):
        self._chk(self.L.admm_hip_upload_state(self.h, _d(x), _d(v)))

    def download_state(self, x=None, v=None):
        self._chk(self.L.admm_hip_download_state(self.h, _d(x), _d(v)))

    def add_gravity(self, g):
        self._chk(self.L.admm_hip_add_gravity(self.h, float(g[0]), float(g[1]), float(g[2])))

    def add_explicit(self, type_, direction, idx=None):
        d = np.ascontiguousarray(direction, dtype=np.float64)
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        n = 0 if ix is None else (ix.size // 3 if type_ == EXPLICIT["WIND"] else ix.size)
        w = C.c_int()
        self._chk(self.L.admm_hip_add_explicit(self.h, type_, _d(d), n, _i(ix), C.byref(w)))
        return w.value

    def set_collision_shapes(self, types, params):
        t = np.ascontiguousarray(types, dtype=np.int32)
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 4)
        self._chk(self.L.admm_hip_set_collision_shapes(self.h, t.size, _i(t), _d(p)))
        self._n_shapes = int(t.size)

    def set_collision_friction(self, mu):
        """one Coulomb coefficient >= 0 per entry of the current shape list (admm_hip_set_collision_friction); before or after
        initialize, between frames.  All zero (the default): the frictionless kernels."""
        m = np.ascontiguousarray(mu, dtype=np.float64).ravel()
        self._chk(self.L.admm_hip_set_collision_friction(self.h, m.size, _d(m)))

    def collision_form(self):
        """which kernels the collision batches launch for the current list (admm_hip_debug_collision_form): 0 frictionless, 1 friction,
        2 moving friction, 3 framed, 4 shell, 5 sheet self-collision, 6 side memory, 7 body self-collision, 8 contact attribution (0-8)"""
        f = C.c_int()
        self._chk(self.L.admm_hip_debug_collision_form(self.h, C.byref(f)))
        return f.value

    def set_collision_frames(self, frames):
        """the rigid frame of every entry of the current shape list (admm_hip_set_collision_frames): [n_shapes][12] = R (row-major), pivot;
        the entry's shape is rotated by R about the pivot, and a box is centred at it.  None: every entry back to the identity."""
        if frames is None:
            self._chk(self.L.admm_hip_set_collision_frames(self.h, self.n_collision_shapes(), None))
            return
        f = np.ascontiguousarray(frames, dtype=np.float64).reshape(-1, 12)
        self._chk(self.L.admm_hip_set_collision_frames(self.h, f.shape[0], _d(f)))

    def n_collision_shapes(self):
        return getattr(self, "_n_shapes", 0)

    def set_collision_motion(self, motion):
        """the rigid motion of every entry of the current shape list (admm_hip_set_collision_motion): [n_shapes][9] = linear velocity,
        angular velocity, pivot, world coordinates; contacts with mu > 0 then stick to the moving surface.  All zero: the default."""
        m = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 9)
        self._chk(self.L.admm_hip_set_collision_motion(self.h, m.shape[0], _d(m)))

    def set_collision_mesh_velocity(self, mesh_id, vel):
        """one velocity per vertex [nv][3] of a registered obstacle mesh (admm_hip_set_collision_mesh_velocity; after initialize, between
        frames), interpolated at a contact for the friction rule; None clears them"""
        if vel is None:
            self._chk(self.L.admm_hip_set_collision_mesh_velocity(self.h, int(mesh_id), 0, None))
            return
        v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
        self._chk(self.L.admm_hip_set_collision_mesh_velocity(self.h, int(mesh_id), v.shape[0], _d(v)))

    def set_body_surface_friction(self, mesh_id, mu):
        """the Coulomb coefficient of a body surface (admm_hip_set_body_surface_friction), for every entry that names it; the surface's
        velocity at a contact comes from its nodes' frame-start v"""
        self._chk(self.L.admm_hip_set_body_surface_friction(self.h, int(mesh_id), float(mu)))

    def add_collision_mesh(self, verts, tris):
        """registers a triangle mesh (before initialize; closed, or an open one: Mesh(verts, tris, half_thickness)) -> its mesh_id for
        SHAPE["MESH"] entries {tx, ty, tz, mesh_id}"""
        m = verts if isinstance(verts, Mesh) else Mesh(verts, tris)
        mid = C.c_int()
        self._chk(self.L.admm_hip_add_collision_mesh(self.h, m.h, C.byref(mid)))
        return mid.value

    def update_collision_mesh(self, mesh_id, verts):
        """new vertex positions [nv][3] for a registered mesh (mesh_id of add_collision_mesh); after initialize on the device, in place"""
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self._chk(self.L.admm_hip_update_collision_mesh(self.h, int(mesh_id), v.shape[0], _d(v)))

    def set_collision_mesh_thickness(self, mesh_id, half_thickness):
        """the half thickness of a registered open mesh (admm_hip_set_collision_mesh_thickness): before or after initialize, between
        frames; captured graphs stay.  A closed mesh, or a value that is not finite and > 0, raises AdmmHipError."""
        self._chk(self.L.admm_hip_set_collision_mesh_thickness(self.h, int(mesh_id), float(half_thickness)))

    def set_collision_mesh_side_memory(self, mesh_id, reach):
        """side memory for a registered open mesh (admm_hip_set_collision_mesh_side_memory; before initialize): every node remembers
        the side of the surface it is on while it is within the reach, and a node that crosses the mid-surface within a frame is put
        back on that side.  reach 0 switches it off.  Keep the reach above closing speed x dt + the half thickness."""
        self._chk(self.L.admm_hip_set_collision_mesh_side_memory(self.h, int(mesh_id), float(reach)))

    def collision_sides(self, mesh_id):
        """-> the side [n_nodes] int32 (+1: where the normals point, -1, 0: none) of every node on a mesh with memory, caller's node
        order (admm_hip_get_collision_sides; after initialize).  Part of a checkpoint beside x, v and u."""
        out = np.empty(self.n_nodes, np.int32)
        self._chk(self.L.admm_hip_get_collision_sides(self.h, int(mesh_id), _i(out)))
        return out

    def set_collision_sides(self, mesh_id, side):
        s = np.ascontiguousarray(side, dtype=np.int32).ravel()
        if s.size != self.n_nodes:
            raise AdmmHipError("set_collision_sides: %d sides given, the system has %d nodes" % (s.size, self.n_nodes))
        self._chk(self.L.admm_hip_set_collision_sides(self.h, int(mesh_id), _i(s)))

    def latch_collision_sides(self):
        """the launches a step begins with (body surfaces, then the latch of every side) from the current x (admm_hip_latch_collision_sides)"""
        self._chk(self.L.admm_hip_latch_collision_sides(self.h))

    def reset_collision_sides(self):
        self._chk(self.L.admm_hip_reset_collision_sides(self.h))

    def add_sheet_surface(self, node_first, node_count, tris, half_thickness, self_collision=False):
        """registers a sheet surface (before initialize): add_body_surface for an open surface of simulated nodes such as a cloth, a
        shell of the given half thickness that follows its nodes and is ignored by them -> its mesh_id.  self_collision: its own nodes
        meet it too, outside their 1-ring (set_sheet_self_collision)."""
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        mid = C.c_int()
        self._chk(self.L.admm_hip_add_sheet_surface(self.h, int(node_first), int(node_count), t.shape[0], _i(t), float(half_thickness), C.byref(mid)))
        if self_collision:
            self.set_sheet_self_collision(mid.value, True)
        return mid.value

    def set_sheet_self_collision(self, mesh_id, on=True):
        """a sheet surface's own nodes collide with it outside their 1-ring (admm_hip_set_sheet_self_collision; before initialize, which
        refuses a sheet with a vertex nearer than the half thickness to a triangle it is not a corner of)"""
        self._chk(self.L.admm_hip_set_sheet_self_collision(self.h, int(mesh_id), 1 if on else 0))

    def add_body_surface(self, node_first, node_count, tris, self_collision=None):
        """registers a body surface (before initialize): a closed mesh of simulated nodes, tris [nt][3] global node ids inside
        [node_first, node_first + node_count), rebuilt from x at every step and ignored by its own nodes -> its mesh_id.
        self_collision = (r, reach, rest_radius): its surface nodes meet it too (set_body_self_collision)."""
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        mid = C.c_int()
        self._chk(self.L.admm_hip_add_body_surface(self.h, int(node_first), int(node_count), t.shape[0], _i(t), C.byref(mid)))
        if self_collision is not None:
            self.set_body_self_collision(mid.value, *self_collision)
        return mid.value

    def set_body_self_collision(self, mesh_id, r, reach, rest_radius):
        """a closed body surface's own surface nodes collide with it (admm_hip_set_body_self_collision; before initialize, which refuses
        a body that the rule would already move where it stands): a node meets the triangles within the reach that are farther than
        rest_radius from it in the rest shape (the positions at add_body_surface), is pushed to distance r outside them, and mirrored
        back out when it has crossed the skin.  r = 0 switches it off.  Keep reach above closing speed x dt + r, rest_radius above the
        reach by the compression the body will see and below the body's thinnest part."""
        self._chk(self.L.admm_hip_set_body_self_collision(self.h, int(mesh_id), float(r), float(reach), float(rest_radius)))

    def set_collision_mesh_owner(self, mesh_id, node_first, node_count):
        """the nodes [node_first, node_first + node_count) skip mesh mesh_id (before initialize; node_count 0 clears the owner)"""
        self._chk(self.L.admm_hip_set_collision_mesh_owner(self.h, int(mesh_id), int(node_first), int(node_count)))

    def body_surface_status(self, mesh_id):
        """-> dict(updated, refused, last_bad_tri): the frame-start updates of a body surface so far (after initialize)"""
        u, r, b = C.c_int64(), C.c_int64(), C.c_int()
        self._chk(self.L.admm_hip_get_body_surface_status(self.h, int(mesh_id), C.byref(u), C.byref(r), C.byref(b)))
        return dict(updated=u.value, refused=r.value, last_bad_tri=b.value)

    def collision_mesh(self, mesh_id):
        """a standalone Mesh copied from registered mesh mesh_id, as registered"""
        h = C.c_void_p()
        self._chk(self.L.admm_hip_collision_mesh_copy(self.h, int(mesh_id), C.byref(h)))
        return Mesh(h)

    def set_gravity(self, which, g):
        self._chk(self.L.admm_hip_set_gravity(self.h, which, float(g[0]), float(g[1]), float(g[2])))

    def set_shard(self, rank, world):
        self._chk(self.L.admm_hip_set_shard(self.h, rank, world))

    # ---- residuals / early exit (extension described at System.cpp:64-65) ----
    def enable_residuals(self, on=True):
        self._chk(self.L.admm_hip_enable_residuals(self.h, 1 if on else 0))

    def set_tolerance(self, eps_r, eps_s, check_every=1):
        self._chk(self.L.admm_hip_set_tolerance(self.h, float(eps_r), float(eps_s), int(check_every)))

    def residuals(self, capacity=256):
        r = np.zeros(capacity); s = np.zeros(capacity); n = C.c_int(0)
        self._chk(self.L.admm_hip_get_residuals(self.h, _d(r), _d(s), capacity, C.byref(n)))
        k = min(n.value, capacity)
        return r[:k], s[:k], n.value

    # ---- energies and the per-iteration objective (extension; include/admm_hip.h) ----
    def energy(self):
        """-> dict(kinetic, gravity, elastic, anchor, n_infinite, batches_skipped) of the state as it stands"""
        t = EnergyTotals()
        self._chk(self.L.admm_hip_energy(self.h, C.byref(t)))
        return t.as_dict()

    def batch_energy(self, batch):
        """-> (total, per_elem [n_local] in read_local's order, n_infinite) of one batch"""
        n = self.local_elements(batch).size
        tot = C.c_double(0.0); ninf = C.c_int64(0); per = np.zeros(n)
        self._chk(self.L.admm_hip_batch_energy(self.h, batch, C.byref(tot), _d(per), C.byref(ninf)))
        return tot.value, per, ninf.value

    def batch_energy_dx(self, batch, dx, out=None):
        """the batch's energy kernel on caller-supplied rows dx [n_local][rows] -> per_elem (written into `out` when given)"""
        dx = np.ascontiguousarray(dx, dtype=np.float64)
        per = np.zeros(self.local_elements(batch).size) if out is None else out
        self._chk(self.L.admm_hip_batch_energy_dx(self.h, batch, _d(dx), _d(per)))
        return per

    def energy_scale(self, batch):
        s = np.zeros(self.local_elements(batch).size)
        self._chk(self.L.admm_hip_read_energy_scale(self.h, batch, _d(s)))
        return s

    # ---- elastic forces and tet stresses: the energies' gradient (extension; include/admm_hip.h) ----
    def batch_gradient(self, batch):
        """-> (g [n_local][rows], corner_forces [n_local][nodes][3], n_nonfinite) of one batch, in read_local's order"""
        kind, _ = self.batches[batch]
        n = self.local_elements(batch).size
        if kind == KIND_GENERIC:
            g = np.zeros((n, 0)); cf = np.zeros((n, 0, 3)); bad = C.c_int64(0)
            self._chk(self.L.admm_hip_batch_gradient(self.h, batch, None, None, C.byref(bad)))
            return g, cf, bad.value
        g = np.zeros((n, KIND_ROWS[kind])); cf = np.zeros((n, KIND_NODES[kind], 3)); bad = C.c_int64(0)
        self._chk(self.L.admm_hip_batch_gradient(self.h, batch, _d(g), _d(cf), C.byref(bad)))
        return g, cf, bad.value

    def batch_gradient_dx(self, batch, dx, out=None):
        """the batch's gradient kernel on caller-supplied rows dx [n_local][rows] -> g (written into `out` when given)"""
        kind, _ = self.batches[batch]
        dx = np.ascontiguousarray(dx, dtype=np.float64)
        g = np.zeros((self.local_elements(batch).size, KIND_ROWS[kind] if kind != KIND_GENERIC else 0)) if out is None else out
        self._chk(self.L.admm_hip_batch_gradient_dx(self.h, batch, _d(dx), _d(g)))
        return g

    def batch_stress(self, batch):
        """-> (stress [n_local][7]: xx, yy, zz, xy, xz, yz, von Mises, n_nonfinite) of a tet batch"""
        st = np.zeros((self.local_elements(batch).size, 7)); bad = C.c_int64(0)
        self._chk(self.L.admm_hip_batch_stress(self.h, batch, _d(st), C.byref(bad)))
        return st, bad.value

    def node_forces(self):
        """-> dict(elastic [n_nodes][3], anchor [n_nodes][3], n_nonfinite, batches_skipped): the internal forces -sum D_i^T dE_i/dd of the
        state as it stands, in the caller's node order; a sharded context returns this rank's share"""
        fe = np.zeros((self.n_nodes, 3)); fa = np.zeros((self.n_nodes, 3)); info = ForceInfo()
        self._chk(self.L.admm_hip_node_forces(self.h, _d(fe), _d(fa), C.byref(info)))
        d = info.as_dict()
        d.update(elastic=fe, anchor=fa)
        return d

    # ---- contact and anchor reactions of the last frame (extension; include/admm_hip.h) ----
    def batch_reaction(self, batch):
        """-> (f [n_local][3], depth [n_local]) of one COLLISION or ANCHOR batch, in read_local's order: the force every element's
        constraint exerted on its node in the last frame, f = w^2 ((z - u) - x), and |u|"""
        n = self.local_elements(batch).size
        f = np.zeros((n, 3)); depth = np.zeros(n)
        self._chk(self.L.admm_hip_batch_reaction(self.h, batch, _d(f), _d(depth)))
        return f, depth

    def node_reactions(self):
        """-> (f_contact [n_nodes][3], f_anchor [n_nodes][3], info) in the caller's node order; info: dict(batches_collision,
        batches_anchor, batches_skipped, n_contacts: the nodes with depth > 0); a sharded context returns this rank's share"""
        fc = np.zeros((self.n_nodes, 3)); fa = np.zeros((self.n_nodes, 3)); info = ReactionInfo()
        self._chk(self.L.admm_hip_node_reactions(self.h, _d(fc), _d(fa), C.byref(info)))
        return fc, fa, info.as_dict()

    def contacts(self, depth_min=1e-10, capacity=None):
        """-> the nodes in contact (depth > depth_min) as a structured array with the fields node, f, point, depth, ascending node index.
        depth_min, a length: above the rounding residue a free node's u carries (a few ulp of |x|), below any penetration you care about.
        capacity (default: all nodes) bounds the records returned; the true count of the last call stays in `last_contact_count`."""
        cap = self.n_nodes if capacity is None else int(capacity)
        rec = np.zeros(max(cap, 0), CONTACT_DTYPE); cnt = C.c_int64(0)
        self._chk(self.L.admm_hip_get_contacts(self.h, float(depth_min), rec.ctypes.data_as(C.c_void_p) if cap > 0 else None, cap, C.byref(cnt)))
        self.last_contact_count = cnt.value
        return rec[:min(cnt.value, max(cap, 0))]

    def contact_resultant(self, pivot=(0.0, 0.0, 0.0), depth_min=1e-10):
        """-> (force [3], torque [3] about `pivot`, count) over the nodes in contact (depth > depth_min)"""
        pv = np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
        out = np.zeros(6); cnt = C.c_int64(0)
        self._chk(self.L.admm_hip_contact_resultant(self.h, float(depth_min), _d(pv), _d(out), C.byref(cnt)))
        return out[:3].copy(), out[3:].copy(), cnt.value

    # ---- contact attribution: what a node touches (extension; include/admm_hip.h) ----
    def enable_contact_attribution(self, on=True):
        """every collision batch records, in every local step, the list entry that last moved each element's candidate and the direction
        of that push (admm_hip_enable_contact_attribution; collision_form() reads 8 while on).  Before or after initialize(), between frames."""
        self._chk(self.L.admm_hip_enable_contact_attribution(self.h, 1 if on else 0))

    def batch_contact_owner(self, batch):
        """-> (entry [n_local] int32, normal [n_local][3]) of one COLLISION batch, in read_local's order: the last entry of the list that
        moved the element's candidate in the last local step (-1: none) and the unit direction of its push (0 where none)"""
        n = self.local_elements(batch).size
        entry = np.zeros(n, np.int32); normal = np.zeros((n, 3))
        self._chk(self.L.admm_hip_batch_contact_owner(self.h, batch, _i(entry), _d(normal)))
        return entry, normal

    def contact_owners(self, depth_min=1e-10, capacity=None):
        """-> the nodes of contacts(depth_min), in its order, as a structured array with the fields node, entry, normal, f_normal,
        f_tangent: the owner entry and normal of the collision element that gives the node its depth, and the node's f_contact split
        about that normal.  capacity as in contacts()."""
        cap = self.n_nodes if capacity is None else int(capacity)
        rec = np.zeros(max(cap, 0), CONTACT_OWNER_DTYPE); cnt = C.c_int64(0)
        self._chk(self.L.admm_hip_get_contact_owners(self.h, float(depth_min), rec.ctypes.data_as(C.c_void_p) if cap > 0 else None, cap, C.byref(cnt)))
        self.last_contact_count = cnt.value
        return rec[:min(cnt.value, max(cap, 0))]

    def entry_resultants(self, pivot=(0.0, 0.0, 0.0), depth_min=1e-10, n_entries=None):
        """-> (force [n_entries + 1][3], torque [n_entries + 1][3] about `pivot`, count [n_entries + 1]): row q over the contacts whose
        owner is entry q of the current shape list, the last row over those that nothing moved in the last local step (entry -1).
        n_entries (default: the current list's length) must be that length."""
        ne = self.n_collision_shapes() if n_entries is None else int(n_entries)
        pv = np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
        out = np.zeros((max(ne, 0) + 1, 6)); cnt = np.zeros(max(ne, 0) + 1, np.int64)
        self._chk(self.L.admm_hip_entry_resultants(self.h, float(depth_min), _d(pv), ne, _d(out), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return out[:, :3].copy(), out[:, 3:].copy(), cnt

    # ---- velocity damping per node group, applied after every frame (extension; include/admm_hip.h) ----
    def add_damping_group(self, node_first=0, node_count=None, drag=0.0, internal=0.0):
        """-> group id.  Nodes [node_first, node_first + node_count) in the caller's order (None: through the last node), rates in 1/s:
        drag (ether drag), internal (removes what is not the group's rigid-body motion).  Before initialize() only."""
        cnt = self.n_nodes - int(node_first) if node_count is None else int(node_count)
        g = C.c_int()
        self._chk(self.L.admm_hip_add_damping_group(self.h, int(node_first), cnt, float(drag), float(internal), C.byref(g)))
        return g.value

    def set_damping(self, group, drag, internal):
        """new rates of one group, in effect from the next step() on"""
        self._chk(self.L.admm_hip_set_damping(self.h, int(group), float(drag), float(internal)))

    def group_moments(self, group):
        """-> dict(mass, com [3], p [3], l [3] about com, inertia [6] = xx yy zz xy xz yz about com, omega [3], t_total, t_rigid, n_nodes,
        degenerate) of one damping group from the device's current x, v"""
        rec = GroupMoments()
        self._chk(self.L.admm_hip_get_group_moments(self.h, int(group), C.byref(rec)))
        return rec.as_dict()

    # ---- pressure chambers: constant and gas-law surface loads, added before every frame (extension; include/admm_hip.h) ----
    def add_pressure_chamber(self, tris, mode="constant", p=0.0, amount=0.0, ambient=0.0):
        """-> chamber id.  tris [nt][3]: oriented triangles over the caller's node ids (outward normals and p > 0 inflate); mode "constant"
        (gauge pressure p) or "gas" (p = amount / V - ambient; the chamber must be closed).  Before initialize() only."""
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        mid, par = _pressure_law(mode, p, amount, ambient)
        c = C.c_int()
        self._chk(self.L.admm_hip_add_pressure_chamber(self.h, t.shape[0], _i(t), mid, _d(par), C.byref(c)))
        return c.value

    def set_pressure(self, chamber, mode="constant", p=0.0, amount=0.0, ambient=0.0):
        """a new law for one chamber, in effect from the next step() on"""
        mid, par = _pressure_law(mode, p, amount, ambient)
        self._chk(self.L.admm_hip_set_pressure(self.h, int(chamber), mid, _d(par)))

    def chamber_state(self, chamber):
        """-> dict(volume, area, area_vector [3], pressure, resultant [3], n_tris, collapsed) of one chamber from the device's current x"""
        rec = ChamberState()
        self._chk(self.L.admm_hip_get_chamber_state(self.h, int(chamber), C.byref(rec)))
        return rec.as_dict()

    # ---- two-way contact: a contact's reaction on the nodes of the surface it landed on (extension; include/admm_hip.h) ----
    def set_surface_reaction(self, mesh_id, share):
        """the share in [0, 1] of a contact's reaction that the corners of the triangle it landed on receive, for one body or sheet
        surface (0: none, the default); needs contact attribution on.  Before or after initialize(), between frames."""
        self._chk(self.L.admm_hip_set_surface_reaction(self.h, int(mesh_id), float(share)))

    def set_surface_reaction_depth(self, depth_min):
        """the depth above which a node counts as in contact for the reaction (default 0), as in contacts(depth_min)"""
        self._chk(self.L.admm_hip_set_surface_reaction_depth(self.h, float(depth_min)))

    def surface_reaction(self, capacity=None):
        """-> (dv [n_nodes][3], records, info) of the last frame: dv what the reaction took off v (0 where nothing landed); one record
        per contact in contacts()' order with the fields node, mesh, tri, corner [3], status (SURFACE_STATUS), weight [3], share; info:
        dict(n_contacts, n_reacting, n_unowned, n_other, n_self)"""
        cap = self.n_nodes if capacity is None else int(capacity)
        dv = np.zeros((self.n_nodes, 3)); rec = np.zeros(max(cap, 0), SURFACE_CONTACT_DTYPE); cnt = C.c_int64(0); info = SurfaceReactionInfo()
        self._chk(self.L.admm_hip_get_surface_reaction(self.h, _d(dv), rec.ctypes.data_as(C.c_void_p) if cap > 0 else None, cap, C.byref(cnt), C.byref(info)))
        return dv, rec[:min(cnt.value, max(cap, 0))], info.as_dict()

    # ---- rigid bodies in the collision list, moved by their contacts (extension; include/admm_hip.h) ----
    def add_rigid_body(self, entry, mass, inertia, com, accel=(0.0, 0.0, 0.0)):
        """-> body id.  Entry `entry` of the current shape list (a sphere, a box or a closed obstacle mesh) becomes a rigid body: mass,
        inertia [6] = xx xy xz yy yz zz about com in the entry's own unrotated coordinates, com [3] in world coordinates, accel [3] a
        constant acceleration (gravity).  Needs contact attribution on.  Before or after initialize()."""
        J = np.ascontiguousarray(inertia, dtype=np.float64).reshape(6)
        c = np.ascontiguousarray(com, dtype=np.float64).reshape(3)
        a = np.ascontiguousarray(accel, dtype=np.float64).reshape(3)
        b = C.c_int()
        self._chk(self.L.admm_hip_add_rigid_body(self.h, int(entry), float(mass), _d(J), _d(c), _d(a), C.byref(b)))
        self.n_rigid = getattr(self, "n_rigid", 0) + 1
        return b.value

    def rigid_body(self, body):
        """-> dict(entry, type, mass, inertia [6], accel [3], c0 [3], par0 [4]): a body's constants, what rigid_query takes"""
        e, t, m = C.c_int(), C.c_int(), C.c_double()
        J, a, c0, p0 = np.zeros(6), np.zeros(3), np.zeros(3), np.zeros(4)
        self._chk(self.L.admm_hip_get_rigid_body(self.h, int(body), C.byref(e), C.byref(t), C.byref(m), _d(J), _d(a), _d(c0), _d(p0)))
        return dict(entry=e.value, type=t.value, mass=m.value, inertia=J, accel=a, c0=c0, par0=p0)

    def rigid_state(self):
        """-> [RigidState] of every body, in the order they were added (admm_hip_get_rigid_state: one synchronisation)"""
        n = getattr(self, "n_rigid", 0)
        recs = (RigidStateRecord * max(n, 1))()
        self._chk(self.L.admm_hip_get_rigid_state(self.h, n, recs))
        return [RigidState(recs[b], self.rigid_body(b)) for b in range(n)]

    def set_rigid_state(self, body, c, q, v, L):
        """c [3], q [4] = (w, x, y, z), v [3], L [3] of one body: a checkpoint, or a kick between frames"""
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(k) for x, k in ((c, 3), (q, 4), (v, 3), (L, 3))]
        self._chk(self.L.admm_hip_set_rigid_state(self.h, int(body), _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3])))

    def set_rigid_accel(self, body, accel):
        """a body's constant acceleration, in effect from the next step() on"""
        a = np.ascontiguousarray(accel, dtype=np.float64).reshape(3)
        self._chk(self.L.admm_hip_set_rigid_accel(self.h, int(body), _d(a)))

    def set_rigid_depth(self, depth_min):
        """the depth above which a node's contact loads a rigid body (default 0), as in entry_resultants(depth_min)"""
        self._chk(self.L.admm_hip_set_rigid_depth(self.h, float(depth_min)))

    # ---- rigid attachments: anchor batches fastened to rigid bodies (extension; include/admm_hip.h) ----
    def attach_anchors(self, batch, body, local=None):
        """The whole ANCHOR batch `batch` is fastened to rigid body `body`: from the next step on the device rewrites its targets from the
        body's pose at the start of every frame and adds the reaction of its active elements to the body's load.  local [n][3]: the
        elements' offsets in the body's own coordinates; None: derived from the batch's current targets and the body's current pose.
        Before or after initialize()."""
        batch = int(batch)
        n = self.batches[batch][1] if 0 <= batch < len(self.batches) else 0
        loc = None if local is None else np.ascontiguousarray(local, dtype=np.float64).reshape(n, 3)
        self._chk(self.L.admm_hip_attach_anchors(self.h, batch, int(body), _d(loc)))

    def detach_anchors(self, batch):
        """the batch's targets stay where the last frame put them; it is a plain moving-anchor batch again"""
        self._chk(self.L.admm_hip_detach_anchors(self.h, int(batch)))

    def attachment(self, batch):
        """-> dict(body (-1: not attached), local [n][3], targets [n][3] as the device holds them now: one synchronisation)"""
        batch = int(batch)
        n = self.batches[batch][1] if 0 <= batch < len(self.batches) else 0
        body = C.c_int(-1); loc = np.zeros((n, 3)); tg = np.zeros((n, 3))
        self._chk(self.L.admm_hip_get_attachment(self.h, batch, C.byref(body), _d(loc), _d(tg)))
        return dict(body=int(body.value), local=loc, targets=tg)

    def attachment_load(self):
        """-> (Fa [n_bodies][3], Ta [n_bodies][3], n_active [n_bodies]): the last frame's attachment row per body, about its centre before
        that frame's integration, as the nodes felt it (the body received the opposite)"""
        n = getattr(self, "n_rigid", 0)
        Fa = np.zeros((max(n, 1), 3)); Ta = np.zeros((max(n, 1), 3)); na = np.zeros(max(n, 1), np.int64)
        self._chk(self.L.admm_hip_get_attachment_load(self.h, n, _d(Fa), _d(Ta), na.ctypes.data_as(C.POINTER(C.c_int64))))
        return Fa[:n], Ta[:n], na[:n]

    def debug_stable_sort(self, keys, key_bound):
        """-> perm [n] int32: the stable ascending order of keys [n] (each in [0, key_bound)) by the reaction's sort kernels alone"""
        k = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
        perm = np.zeros(k.size, np.int32)
        self._chk(self.L.admm_hip_debug_stable_sort(self.h, k.size, _i(k), int(key_bound), _i(perm)))
        return perm

    def enable_objective(self, on=True):
        self._chk(self.L.admm_hip_enable_objective(self.h, 1 if on else 0))

    def objective(self, capacity=256):
        """-> (inertia, elastic, n_iters) of the last step's ADMM iterations; the objective is inertia + elastic"""
        a = np.zeros(capacity); e = np.zeros(capacity); n = C.c_int(0)
        self._chk(self.L.admm_hip_get_objective(self.h, _d(a), _d(e), capacity, C.byref(n)))
        k = min(n.value, capacity)
        return a[:k], e[:k], n.value

    # ---- Anderson acceleration of the ADMM iteration (extension; include/admm_hip.h) ----
    def set_acceleration(self, window):
        """window m of the history, 0 .. 8; 0 (the default) switches acceleration off"""
        self._chk(self.L.admm_hip_set_acceleration(self.h, int(window)))

    def acceleration_log(self, capacity=512):
        """-> one dict per ADMM iteration of the last step: rho, accepted, m_used, extrapolated, solve_failed, theta [m_used],
        gram [m_used][m_used] and rhs [m_used] (the system the device solved, before regularisation; differences oldest first)"""
        rec = (AccelerationRecord * max(capacity, 1))(); n = C.c_int(0)
        self._chk(self.L.admm_hip_get_acceleration_log(self.h, rec, capacity, C.byref(n)))
        out = []
        for r in rec[:min(n.value, capacity)]:
            mk = r.m_used
            out.append(dict(rho=r.rho, accepted=bool(r.accepted), m_used=mk, extrapolated=bool(r.extrapolated), solve_failed=bool(r.solve_failed),
                            theta=np.array(r.theta[:mk]), gram=np.array(r.gram[:]).reshape(8, 8)[:mk, :mk].copy(), rhs=np.array(r.rhs[:mk])))
        return out

    def acceleration_default(self, batch):
        """-> dict(z, u) [n_local][rows]: the stored default s_def of one batch (the last accepted local-step output), in read_local's layout"""
        kind, _ = self.batches[batch]
        n = self.local_elements(batch).size
        rows = KIND_ROWS[kind] if kind != KIND_GENERIC else 0
        z = np.zeros((n, rows)); u = np.zeros((n, rows))
        self._chk(self.L.admm_hip_get_acceleration_default(self.h, batch, _d(z), _d(u)))
        return dict(z=z, u=u)

    def set_allreduce(self, pyfunc):
        """pyfunc(dev_ptr:int, count:int, stream:int) -> 0 on success."""
        def tramp(user, buf, count, stream):
            try:
                return int(pyfunc(buf or 0, int(count), stream or 0) or 0)
            except Exception as e:  # never let an exception cross the C boundary
                print("allreduce hook raised:", e)
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        self._chk(self.L.admm_hip_set_allreduce(self.h, self._cb, None))

    def initialize(self):
        self._chk(self.L.admm_hip_finalize(self.h))
        return True

    def recompute_weights(self):
        self._chk(self.L.admm_hip_recompute_weights(self.h))

    def set_weights(self, batch, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self.L.admm_hip_set_weights(self.h, batch, _d(w)))

    def update_anchors(self, batch, targets=None, active=None):
        tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.float64)
        ac = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        self._chk(self.L.admm_hip_update_anchors(self.h, batch, _d(tg), _i(ac)))

    # ---- stepping (System.hpp:65) ----
    def step(self, admm_iters):
        self._chk(self.L.admm_hip_step(self.h, int(admm_iters)))

    def sync(self):
        self._chk(self.L.admm_hip_sync(self.h))

    # ---- state ----
    def _getn(self, fn):
        a = np.zeros(3 * self.n_nodes)
        self._chk(fn(self.h, _d(a)))
        return a

    @property
    def m_x(self):
        return self._getn(self.L.admm_hip_get_x)

    @m_x.setter
    def m_x(self, val):
        val = np.ascontiguousarray(val, dtype=np.float64).ravel()
        assert val.size == 3 * self.n_nodes
        self._chk(self.L.admm_hip_set_x(self.h, _d(val)))

    @property
    def m_v(self):
        return self._getn(self.L.admm_hip_get_v)

    @m_v.setter
    def m_v(self, val):
        val = np.ascontiguousarray(val, dtype=np.float64).ravel()
        self._chk(self.L.admm_hip_set_v(self.h, _d(val)))

    # ---- parity / introspection ----
    def info(self):
        inf = Info()
        self._chk(self.L.admm_hip_get_info(self.h, C.byref(inf)))
        return inf.as_dict()

    def local_elements(self, batch):
        """this rank's elements of a batch (reference order): the rows of read_local / write_local"""
        n = C.c_int(0)
        self._chk(self.L.admm_hip_local_elements(self.h, batch, None, 0, C.byref(n)))
        ids = np.zeros(n.value, np.int32)
        self._chk(self.L.admm_hip_local_elements(self.h, batch, _i(ids), n.value, C.byref(n)))
        return ids

    def local_range(self, batch):
        """contiguous sharding: [first, end) of this rank's elements"""
        ids = self.local_elements(batch)
        if ids.size == 0:
            kind, n = self.batches[batch]
            inf = self.info()
            return n * inf["rank"] // inf["world"], n * inf["rank"] // inf["world"]
        assert np.array_equal(ids, np.arange(ids[0], ids[0] + ids.size)), "not a contiguous shard"
        return int(ids[0]), int(ids[0]) + ids.size

    def node_owner(self):
        o = np.zeros(self.n_nodes, np.int32)
        self._chk(self.L.admm_hip_debug_node_owner(self.h, _i(o)))
        return o

    def node_supernode(self):
        """-> (supernode of each node's column, the column's place inside it, every supernode's parent (-1: a root))"""
        sn = np.zeros(self.n_nodes, np.int32); col = np.zeros(self.n_nodes, np.int32)
        par = np.zeros(max(1, self.info()["n_supernodes"]), np.int32)
        self._chk(self.L.admm_hip_debug_node_supernode(self.h, _i(sn), _i(col), _i(par)))
        return sn, col, par[:self.info()["n_supernodes"]]

    def set_shard_mode(self, mode):
        self._chk(self.L.admm_hip_set_shard_mode(self.h, SHARD[mode] if isinstance(mode, str) else int(mode)))

    def set_factor_local(self, on):
        """Rank-local factorization under subtree sharding (default on): initialize() / recompute_weights() are then collective calls."""
        self._chk(self.L.admm_hip_set_factor_local(self.h, int(bool(on))))

    def read_local(self, batch):
        kind, _ = self.batches[batch]
        if kind == KIND_GENERIC:     # u, z of this rank's user forces, element after element
            nr = int(self._generic_rows[batch][self.local_elements(batch)].sum())
            u = np.zeros(nr); z = np.zeros(nr)
            self._chk(self.L.admm_hip_read_local(self.h, batch, _d(u), _d(z), None, None))
            return dict(u=u, z=z)
        n = self.local_elements(batch).size
        rows = KIND_ROWS[kind]
        u = np.zeros((n, rows)); z = np.zeros((n, rows))
        st = np.zeros((n, 4 if KIND_STATE[kind] else 3)); it = np.zeros(n, np.int32)
        self._chk(self.L.admm_hip_read_local(self.h, batch, _d(u), _d(z), _d(st), _i(it)))
        return dict(u=u, z=z, state=st, n_iters=it)

    def write_local(self, batch, u=None, state=None):
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        state = None if state is None else np.ascontiguousarray(state, dtype=np.float64)
        self._chk(self.L.admm_hip_write_local(self.h, batch, _d(u), _d(state)))

    def read_rest(self, batch):
        kind, n = self.batches[batch]
        w = np.zeros(n); rest = np.zeros((n, 12)); g = np.zeros(n, np.int32)
        self._chk(self.L.admm_hip_read_rest(self.h, batch, _d(w), _d(rest), _i(g)))
        return dict(weight=w, rest=rest, global_idx=g)

    def local_step_only(self, x_cur):
        x_cur = np.ascontiguousarray(x_cur, dtype=np.float64).ravel()
        self._chk(self.L.admm_hip_local_step_only(self.h, _d(x_cur)))

    def debug_rhs(self):
        """the right-hand side b = M x_bar + dt^2 D^T W^2 (z - u) the last local step assembled (this rank's, before any all-reduce)"""
        return self._getn(self.L.admm_hip_debug_rhs)

    def local_step_dx(self, batch, dx):
        dx = np.ascontiguousarray(dx, dtype=np.float64)
        self._chk(self.L.admm_hip_local_step_dx(self.h, batch, _d(dx)))

    def solve_only(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        x = np.zeros_like(b)
        self._chk(self.L.admm_hip_solve_only(self.h, _d(b), _d(x)))
        return x

    def apply_A(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.zeros_like(x)
        self._chk(self.L.admm_hip_apply_A(self.h, _d(x), _d(y)))
        return y

    def debug_math(self, op, x):
        """one function of csrc/local_math.hpp as the device executes it, one lane per record (parity tests; include/admm_hip.h
        admm_hip_debug_math lists the ops): x (n, IN) -> (n, OUT); record i runs on lane i % 64 of wave i / 64"""
        n_in, n_out = DEBUG_MATH_SHAPES[int(op)]
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n_in:
            raise ValueError("debug_math op %d takes an (n, %d) array, got %s" % (op, n_in, x.shape))
        y = np.empty((x.shape[0], n_out))
        self._chk(self.L.admm_hip_debug_math(self.h, int(op), x.shape[0], _d(x), _d(y)))
        return y

    def debug_gemm(self, A, B, Cm, m, n, k, flags=0, alpha=1.0, beta=0.0):
        """gemm_f64_kernel on column-major (Fortran-ordered) 2-D arrays; Cm is updated in place and returned."""
        A = np.asfortranarray(A, dtype=np.float64); B = np.asfortranarray(B, dtype=np.float64)
        assert Cm.flags.f_contiguous and Cm.dtype == np.float64
        self._chk(self.L.admm_hip_debug_gemm(self.h, m, n, k, A.shape[0], B.shape[0], Cm.shape[0], flags, alpha, beta,
                                             _d(A), A.size, _d(B), B.size, _d(Cm), Cm.size))
        return Cm

    def debug_potrf_inv(self, blk):
        """potrf_inv_kernel: (L, L^-1) of a symmetric positive definite block of at most 64 rows."""
        w = blk.shape[0]
        Lm = np.asfortranarray(blk, dtype=np.float64).copy(order="F")
        X = np.zeros_like(Lm, order="F")
        self._chk(self.L.admm_hip_debug_potrf_inv(self.h, w, w, _d(Lm), _d(X)))
        return np.tril(Lm), X

    def debug_panel_solve_host(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        x = np.zeros_like(b)
        self._chk(self.L.admm_hip_debug_panel_solve_host(self.h, _d(b), _d(x)))
        return x

    def keep_z(self, on=True):
        """admm_hip_keep_z: whether admm_hip_step stores the tet batches' z (read_local) -- off for production frames."""
        self._chk(self.L.admm_hip_keep_z(self.h, 1 if on else 0))

    def enable_timing(self, on=True):
        self._chk(self.L.admm_hip_enable_timing(self.h, int(on)))

    def timing(self):
        t = Timing()
        self._chk(self.L.admm_hip_get_timing(self.h, C.byref(t)))
        return t.as_dict()

    def timing_previous(self):
        """phase times of the step BEFORE the last one (read after the next step has been queued: no idle GPU between frames)"""
        t = Timing()
        self._chk(self.L.admm_hip_get_timing_previous(self.h, C.byref(t)))
        return t.as_dict()


class RankErrors(AdmmHipError):
    """A collective call of several ranks' contexts (call_together) failed on at least one rank.  errors[r]: rank r's exception,
    None where the call returned, an AdmmHipError "still inside" where it had not returned when call_together gave up."""

    def __init__(self, call, errors):
        self.errors = errors
        super().__init__("%s: %s" % (call, "; ".join("rank %d %s" % (r, "returned OK" if e is None else "raised: %s" % e)
                                                     for r, e in enumerate(errors))))


def call_together(systems, call, timeout=3600.0, grace=30.0):
    """systems[r].<call>() of several ranks' contexts living in ONE process, each from its own thread -- for the collective calls
    (initialize / recompute_weights under rank-local factorization), where every rank must be inside the call at the same time.
    Returns when every rank has returned.  ONE deadline, `timeout` seconds from the start, covers all ranks; once a rank has raised,
    the others get at most `grace` more seconds to come out.  Any failure raises RankErrors carrying every rank's outcome."""
    import threading
    import time
    n = len(systems)
    errors, done, first_fail = [None] * n, [False] * n, []
    cv = threading.Condition()

    def run(r):
        try:
            getattr(systems[r], call)()
        except BaseException as e:  # noqa: BLE001
            errors[r] = e
        with cv:
            done[r] = True
            if errors[r] is not None and not first_fail:
                first_fail.append(time.monotonic())
            cv.notify_all()
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(n)]
    deadline = time.monotonic() + timeout
    for t in th:
        t.start()
    with cv:
        while not all(done):
            end = min(deadline, first_fail[0] + grace) if first_fail else deadline
            left = end - time.monotonic()
            if left <= 0:
                break
            cv.wait(left)
        hung = [r for r in range(n) if not done[r]]
        out = list(errors)
    for r in hung:
        out[r] = AdmmHipError("still inside %s() %s" % (call, "%g s after another rank failed" % grace if first_fail else "after %g s" % timeout))
    if any(e is not None for e in out):
        raise RankErrors(call, out)


def initialize_together(systems, timeout=3600.0, grace=30.0):
    """initialize() of several ranks' contexts living in ONE process (tests, tools/ranks_one_gpu.py), each from its own thread:
    under rank-local factorization (subtree shards, the default) admm_hip_finalize is a collective call -- the ranks meet in the
    all-reduce of the subtree roots' update matrices -- exactly like System::initialize() of N real processes.  See call_together."""
    call_together(systems, "initialize", timeout, grace)


def make_bar_system(nx, ny, nz, kind=KIND["TET_NH"], mu=1e5, lam=1e5, max_iter=5, density=1000.0, h=0.05, dt=0.04,
                    gravity=(0.0, -9.8, 0.0), device_id=0, rank=0, world=1, stream=None, shard_mode=None):
    """The synthetic bar of BASELINE.md section 4 config 4: tets first, then
    StaticAnchors on the k = 0 face, gravity, lumped density-weighted mass."""
    x, tets = meshgen.bar(nx, ny, nz, h)
    m = meshgen.lumped_tet_mass(x, tets, density)
    s = System(device_id=device_id, stream=stream)
    s.set_timestep(dt)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(kind, tets, [mu, lam, max_iter])
    s.add_forces(KIND["ANCHOR"], meshgen.bar_anchor_nodes(nx, ny), [-1.0, 1.0])
    s.add_gravity(gravity)
    if world > 1:
        s.set_shard(rank, world)
        if shard_mode is not None:
            s.set_shard_mode(shard_mode)
    s.n_tets = tets.shape[0]
    return s


def make_mixed_system(nx, ny, nz, cloth_w, cloth_l, device_id=0, dt=0.04, rank=0, world=1, stream=None, shard_mode=None):
    """BASELINE.md section 4 config 5 ("mixed scene"): a bar whose lower half (in z) is Neo-Hookean and
    upper half StVK (tets first), then a sym-plane cloth with LimitedTriangleStrain (k=100,
    limits .95/1.05) + BendForce (k=20) hanging from two corner anchors, bar face anchored, gravity.
    Returns (system, description dict with the arrays the oracle needs)."""
    x, tets = meshgen.bar(nx, ny, nz)
    m = meshgen.lumped_tet_mass(x, tets, 1000.0)
    half = tets.shape[0] // 2
    xc, tris = meshgen.sym_plane(cloth_w, cloth_l, size=1.0)
    xc = xc + np.array([3.0, 1.0, 0.0])
    hinges = meshgen.bend_hinges(tris)
    off = x.shape[0]
    X = np.concatenate([x, xc])
    M = np.concatenate([m, np.full(xc.shape[0], 0.5 / xc.shape[0])])
    s = System(device_id=device_id, stream=stream)
    s.set_timestep(dt)
    s.add_nodes(X.ravel(), np.repeat(M, 3))
    desc = dict(X=X, M=M, forces=[
        ("TET_NH", tets[:half], [1e5, 1e5, 5]), ("TET_STVK", tets[half:], [1e5, 1e5, 5]),
        ("TRI_STRAIN", tris + off, [100.0, 0.95, 1.05, 1.0]), ("BEND", hinges + off, [20.0]),
        ("ANCHOR", np.concatenate([meshgen.bar_anchor_nodes(nx, ny), np.array([off, off + cloth_w], dtype=np.int32)]), [-1.0, 1.0])])
    for name, idx, par in desc["forces"]:
        s.add_forces(KIND[name], idx, par)
    s.add_gravity((0.0, -9.8, 0.0))
    if world > 1:
        s.set_shard(rank, world)
        if shard_mode is not None:
            s.set_shard_mode(shard_mode)
    s.n_elements = tets.shape[0] + tris.shape[0]
    return s, desc
