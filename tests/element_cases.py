"""What tests/test_energy.py and tests/test_element_forces.py share: the elements' inputs, the long-double helpers, the scenes, D_i x in
the documented accumulation order and the bit comparisons.  A plain module, imported like checkers.  What differs between the two files
(the material table PARAMS, rest_rows, ld_energy, sized_system) stays with them; mixed_forces is handed its caller's PARAMS."""
import numpy as np
import pytest

from checkers import KIND, KIND_NODES

LD = np.longdouble
needs_ld = pytest.mark.skipif(np.finfo(LD).eps > 2.0 ** -63, reason="np.longdouble has no extended precision on this host")

TET_KINDS = ("TET_NH", "TET_STVK", "TET_LINEAR", "TET_VOLUME")
TRI_KINDS = ("TRI_FUNG", "TRI_STRAIN", "TRI_AREA")
EVALUATED = TET_KINDS + TRI_KINDS + ("SPRING", "BEND")
SCALE = 0.37           # the elements' scale s in the host tests (a rest volume; any positive number)
SPRING_L = 0.8
BEND_ALPHA = (0.45, 0.55, -0.6, -0.4)
BAR = (3, 3, 5)          # 270 tets, 96 nodes
CLOTH = (6, 5)           # 120 triangles, 72 nodes
H = 0.05
DT = 0.04
G = (0.0, -9.8, 0.0)


def _pkg():
    from __graft_entry__ import load_package
    return load_package()


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def tet_inputs():
    """d = I + 0.3 N(0, 1), 4096 of them, seed 0 (element-major rows: column-major 3x3), then by hand: rest, uniform scale 0.5 / 1.2 / 3,
    rank-deficient, exactly inverted"""
    rng = np.random.default_rng(0)
    I = np.eye(3).T.reshape(9)
    d = I + 0.3 * rng.standard_normal((4096, 9))
    hand = [I, 0.5 * I, 1.2 * I, 3.0 * I]
    rd = np.array([[1.0, 0.2, 0.0], [0.0, 1.1, 0.3], [0.0, 0.0, 0.0]]).T.reshape(9)      # rank 2
    r1 = np.outer([1.0, 0.5, -0.2], [0.3, 1.0, 0.7]).T.reshape(9)                          # rank 1
    inv = np.diag([1.0, 1.0, -1.0]).T.reshape(9)                                           # exactly inverted
    inv2 = np.array([[0.9, 0.1, 0.0], [0.0, -1.2, 0.2], [0.1, 0.0, 1.1]]).T.reshape(9)
    return np.vstack([d] + [np.asarray(h)[None] for h in hand + [rd, r1, inv, inv2]])


def tri_inputs():
    rng = np.random.default_rng(0)
    I = np.array([1.0, 0, 0, 0, 1.0, 0])
    d = I + 0.3 * rng.standard_normal((4096, 6))
    hand = [I, 0.5 * I, 1.2 * I, 3.0 * I, np.array([1.0, 0.5, 0.0, 2.0, 1.0, 0.0]), np.array([1.0, 0.2, 0.3, 0, 0, 0.0]),
            np.array([0.0, 1.0, 0.0, 1.0, 0.0, 0.0]), 20.0 * I]
    return np.vstack([d] + [np.asarray(h)[None] for h in hand])


def spring_inputs():
    rng = np.random.default_rng(0)
    d = 0.8 * np.array([1.0, 0, 0]) + 0.3 * rng.standard_normal((4096, 3))
    return np.vstack([d, [[0.8, 0, 0]], [[0.4, 0, 0]], [[0, 0, 2.4]], [[0, 0, 0]]])


def bend_inputs():
    rng = np.random.default_rng(0)
    base = np.array([0.5, 0.0, 0.5, 0.5, 0.0, -0.5, 1.0, 0.0, 0.0])
    d = base + 0.3 * rng.standard_normal((4096, 9))
    return np.vstack([d, base[None], 0.5 * base[None], 3.0 * base[None]])


def inputs(kind):
    if kind == "TET_VOLUME":
        # without the rank-1 case: TetVolume's four steps divide by |grad det|^2 = (s1 s2)^2 + (s0 s2)^2 + (s0 s1)^2, which for two zero
        # singular values is the square of rounding noise (1e-34): the projection there is decided by the SVD's last bits in any precision.
        # The rank-2 case stays.
        d = tet_inputs()
        return np.delete(d, 4096 + 5, axis=0)
    if kind in TET_KINDS:
        return tet_inputs()
    if kind in TRI_KINDS:
        return tri_inputs()
    return spring_inputs() if kind == "SPRING" else bend_inputs()


# ---------------------------------------------------------------------------------------------------------------------------------
# long-double helpers of the restatements (ld_energy in the two test files)
# ---------------------------------------------------------------------------------------------------------------------------------
def ld_singular_values(A):
    """singular values of A [n][rows][cols] (cols <= rows) in long double, descending: one-sided Jacobi (Hestenes), which orthogonalises
    the columns by plane rotations and is accurate to the precision for small singular values too; the values are the columns' norms"""
    A = np.array(A, dtype=LD)
    cols = A.shape[2]
    for _ in range(12):
        for p in range(cols - 1):
            for q in range(p + 1, cols):
                ap, aq = A[:, :, p].copy(), A[:, :, q].copy()
                al, be, ga = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
                rot = np.abs(ga) > LD(1e-22) * np.sqrt(al * be)
                g = np.where(rot, ga, LD(1))
                zeta = (be - al) / (LD(2) * g)
                t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(LD(1) + zeta * zeta))
                c = LD(1) / np.sqrt(LD(1) + t * t)
                s = c * t
                c = np.where(rot, c, LD(1))[:, None]; s = np.where(rot, s, LD(0))[:, None]
                A[:, :, p] = c * ap - s * aq
                A[:, :, q] = s * ap + c * aq
    sv = np.sqrt((A * A).sum(1))
    return -np.sort(-sv, axis=1)


def ld_det3(M):
    return (M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]) - M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0])
            + M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes and D_i x in the documented accumulation order
# ---------------------------------------------------------------------------------------------------------------------------------
def cloth_mesh():
    mg = _pkg().meshgen
    x, tris = mg.sym_plane(*CLOTH)
    hinges = mg.bend_hinges(tris)
    e = np.sort(np.vstack([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    edges = np.unique(e, axis=0).astype(np.int32)
    return x, tris, hinges, edges


def element_dx(kind, idx, rest, x):
    """D_i x of every element, element-major [n][rows], with the device's bits: tets and triangles accumulate B(c, r) x_c from 0.0 over the
    corners in ascending node order (a rounded product, then a rounded sum: numpy's float64 does exactly that); springs and hinges are
    plain differences"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]])
    n = idx.shape[0]
    if kind in TET_KINDS or kind in TRI_KINDS:
        nc, nr = (4, 3) if kind in TET_KINDS else (3, 2)
        order = np.argsort(idx, axis=1, kind="stable")
        out = np.zeros((n, 3 * nr))
        ar = np.arange(n)
        for r in range(nr):
            for j in range(3):
                acc = np.zeros(n)
                for k in range(nc):
                    c = order[:, k]
                    acc = acc + rest[ar, c + nc * r] * x[idx[ar, c], j]
                out[:, 3 * r + j] = acc
        return out
    if kind == "SPRING":
        return x[idx[:, 0]] - x[idx[:, 1]]
    if kind == "BEND":
        return np.hstack([x[idx[:, 0]] - x[idx[:, 2]], x[idx[:, 3]] - x[idx[:, 2]], x[idx[:, 1]] - x[idx[:, 2]]])
    raise ValueError(kind)


def mixed_forces(PARAMS):
    """every kind at once: the bar's tets in four materials, the cloth's triangles in three, its hinges and edge springs, anchors, and a
    collision batch over all nodes -> (X, M3, [(kind, idx, params)])"""
    mg = _pkg().meshgen
    xb, tets = mg.bar(*BAR, h=H)
    xc, tris, hinges, edges = cloth_mesh()
    off = xb.shape[0]
    X = np.concatenate([xb, 0.3 * xc + np.array([0.5, 0.1, 0.0])])
    M = np.concatenate([mg.lumped_tet_mass(xb, tets, 1000.0), np.full(xc.shape[0], 0.5 / xc.shape[0])])
    anchors = np.concatenate([mg.bar_anchor_nodes(BAR[0], BAR[1]), np.array([off, off + CLOTH[0]], dtype=np.int32)]).astype(np.int32)
    forces = [("TET_NH", tets[:70], PARAMS["TET_NH"]), ("TET_STVK", tets[70:140], PARAMS["TET_STVK"]), ("TET_LINEAR", tets[140:205], PARAMS["TET_LINEAR"]),
              ("TET_VOLUME", tets[205:], PARAMS["TET_VOLUME"]), ("TRI_STRAIN", tris[:40] + off, PARAMS["TRI_STRAIN"]), ("TRI_AREA", tris[40:80] + off, PARAMS["TRI_AREA"]),
              ("TRI_FUNG", tris[80:] + off, PARAMS["TRI_FUNG"]), ("BEND", hinges + off, PARAMS["BEND"]), ("SPRING", edges + off, PARAMS["SPRING"]),
              ("ANCHOR", anchors, [-1.0, 1.0]), ("COLLISION", np.arange(X.shape[0], dtype=np.int32), [32.0])]
    return X, np.repeat(M, 3), forces


def build_system(X, M3, forces, device_id=0, gravity=G, shapes=True, rank=0, world=1):
    pkg = _pkg()
    s = pkg.System(device_id=device_id)
    s.set_timestep(DT)
    s.add_nodes(np.ascontiguousarray(X).ravel(), M3)
    for kind, idx, par in forces:
        s.add_forces(KIND[kind], np.ascontiguousarray(idx, dtype=np.int32), par)
    if gravity is not None:
        s.add_gravity(gravity)
    if shapes and any(k == "COLLISION" for k, _, _ in forces):
        s.set_collision_shapes([pkg.SHAPE["FLOOR"]], [[0.0, -5.0, 0.0, 0.0]])
    if world > 1:
        s.set_shard(rank, world)
    return s


def deform(X, amp=0.04, fold=False):
    """a smooth deformation of the rest positions; fold: one bar node pulled far through its neighbours, which inverts the tets around it"""
    x = np.asarray(X, dtype=np.float64).copy()
    k = np.arange(x.size, dtype=np.float64).reshape(x.shape)
    x = x * (1.0 + amp * np.sin(1.7 * k)) + 0.3 * amp * H * np.cos(0.9 * k)
    if fold:
        x[5] = x[5] + np.array([3.0 * H, 2.5 * H, 2.0 * H])
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# the solver's state and bit comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def _state(s, forces):
    out = [s.m_x, s.m_v]
    for b in range(len(forces)):
        loc = s.read_local(b)
        out += [loc["u"], loc["state"], loc["n_iters"].astype(np.float64)]
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))
