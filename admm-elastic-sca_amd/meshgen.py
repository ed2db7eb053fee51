"""Synthetic scene generators for the configurations of BASELINE.md section 4 /
SURVEY.md section 8(d).  Pure numpy, deterministic, seed-free.

`bar()` is the "synthetic NH bar" of config 4: an nx*ny*nz grid of cubes with
spacing h, node id = i + (nx+1)*(j + (ny+1)*k), each cube split into 6 Kuhn
tets (one per permutation of the axes, order 012,021,102,120,201,210; vertices
= the cube corner (i,j,k) followed by successive +1 steps along the permuted
axes; last two vertices swapped when the signed volume is negative), tets
emitted cube-major (i fastest).  32x32x163 gives 1 001 472 tets / 178 596 nodes.
"""
import itertools

import numpy as np

KUHN_PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def bar(nx, ny, nz, h=0.05):
    """Returns (x [n,3] float64, tets [m,4] int32)."""
    gx, gy, gz = nx + 1, ny + 1, nz + 1
    k, j, i = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    x = np.stack([i.ravel() * h, j.ravel() * h, k.ravel() * h], axis=1).astype(np.float64)

    ck, cj, ci = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    corner = np.stack([ci.ravel(), cj.ravel(), ck.ravel()], axis=1)  # cube-major, i fastest
    ncube = corner.shape[0]
    tets = np.empty((ncube, 6, 4), dtype=np.int64)
    strides = np.array([1, gx, gx * gy], dtype=np.int64)
    for p, perm in enumerate(KUHN_PERMS):
        c = corner.copy()
        tets[:, p, 0] = c @ strides
        for s, ax in enumerate(perm):
            c[:, ax] += 1
            tets[:, p, s + 1] = c @ strides
    tets = tets.reshape(-1, 4)
    # orientation: swap the last two vertices where the signed volume is negative
    v0, v1, v2, v3 = (x[tets[:, a]] for a in range(4))
    vol = np.einsum("ij,ij->i", np.cross(v1 - v0, v2 - v0), v3 - v0)
    neg = vol < 0
    tets[neg, 2], tets[neg, 3] = tets[neg, 3].copy(), tets[neg, 2].copy()
    return x, tets.astype(np.int32)


def slotted_bar(nx, ny, nz, slot_from, h=0.05):
    """bar(nx, ny, nz, h) without the cubes whose j == ny // 2 and k >= slot_from: two arms one cell apart, joined by a spine (a
    gripper, a tuning fork) -> (x, tets): the positions of bar (nodes inside the slot that no tet uses included) and the kept tets in
    bar's order."""
    x, tets = bar(nx, ny, nz, h)
    ck, cj, _ = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cut = ((cj.ravel() == ny // 2) & (ck.ravel() >= slot_from))      # cube-major, i fastest, six tets a cube: bar's order
    return x, np.ascontiguousarray(tets[~np.repeat(cut, 6)])


def lumped_tet_mass(x, tets, density):
    """rho * vol / 4 to each corner (ForceBuilder density-weighted mass,
    reference src/ForceBuilder.hpp:191-303); returns [n] per-node mass."""
    v0, v1, v2, v3 = (x[tets[:, a]] for a in range(4))
    vol = np.abs(np.einsum("ij,ij->i", np.cross(v1 - v0, v2 - v0), v3 - v0)) / 6.0
    m = np.zeros(x.shape[0])
    np.add.at(m, tets.ravel(), np.repeat(density * vol / 4.0, 4))
    return m


def tet_surface(tets, x=None):
    """the boundary of a tet mesh -> tris [nt][3] int32: the faces that occur once, in the tets' order (faces opposite corners 0, 1, 2, 3),
    each oriented away from its tet's fourth corner -- by the corner order of a positively oriented tet (meshgen.bar's), or, given the
    positions x [n][3], by the geometry whatever the tets' orientation"""
    T = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    # opposite corner 0, 1, 2, 3: counter-clockwise seen from outside when (v1 - v0) x (v2 - v0) . (v3 - v0) > 0
    F = T[:, [[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]]].reshape(-1, 3)
    O = T.reshape(-1)
    _, inv, cnt = np.unique(np.sort(F, axis=1), axis=0, return_inverse=True, return_counts=True)
    once = cnt[inv.reshape(-1)] == 1
    F, O = F[once], O[once]
    if x is not None:
        P = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        n = np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])
        inward = np.einsum("ij,ij->i", n, P[O] - P[F[:, 0]]) > 0
        F[inward] = F[inward][:, [0, 2, 1]]
    return np.ascontiguousarray(F, dtype=np.int32)


def bar_anchor_nodes(nx, ny):
    """node ids of the k = 0 face."""
    return np.arange((nx + 1) * (ny + 1), dtype=np.int32)


def sym_plane(w, l, size=1.0):
    """A (w x l)-cell 'symmetric plane' cloth: every cell has a centre vertex
    and 4 triangles (4*w*l tris, (w+1)(l+1)+w*l nodes) in the xz-plane, as
    trimesh2's make_sym_plane lays it out (reference
    deps/mclscene/deps/trimesh2/include/TriMeshBuilder.h:116-171).  Geometry is
    generated in float64 here (the reference rounds vertices to float)."""
    nv = (w + 1) * (l + 1)
    ii, jj = np.meshgrid(np.arange(w + 1), np.arange(l + 1), indexing="xy")
    gx = (ii.ravel() / w - 0.5) * size
    gz = (jj.ravel() / l - 0.5) * size * l / w
    ci, cj = np.meshgrid(np.arange(w), np.arange(l), indexing="xy")
    cx = ((ci.ravel() + 0.5) / w - 0.5) * size
    cz = ((cj.ravel() + 0.5) / l - 0.5) * size * l / w
    x = np.zeros((nv + w * l, 3))
    x[:nv, 0] = gx; x[:nv, 2] = gz
    x[nv:, 0] = cx; x[nv:, 2] = cz
    tris = []
    for j, i in itertools.product(range(l), range(w)):
        a = i + (w + 1) * j; b = a + 1; c = a + (w + 1); d = c + 1; m = nv + i + w * j
        tris += [(a, b, m), (b, d, m), (d, c, m), (c, a, m)]
    return x, np.array(tris, dtype=np.int32)


def sheet_tris(w, l, node_first=0):
    """The triangles of a (w x l)-cell sym_plane cloth as a sheet surface: global node ids for a cloth whose nodes start at
    node_first (System.add_sheet_surface), in sym_plane's order and (consistent) orientation."""
    return (sym_plane(w, l)[1] + np.int32(node_first)).astype(np.int32)


def folded_strip(w, l, gap):
    """A (w x l)-cell sym_plane strip (cell size h = 1 / w) bent into a U whose two flat flaps are `gap` apart: the lower flap in the
    plane y = 0, a straight fold of height gap, the upper flap in the plane y = gap running back over the lower one.  A vertex at arc
    length s along the strip (s = j / w for grid row j, (j + 0.5) / w for the centre vertices of cell row j) sits on the path
    (y, z) = (0, s) for s <= a,  (s - a, a) for a < s <= a + gap,  (gap, a - (s - a - gap)) beyond,  a = (l // 2 + 1 / 16) / w:
    the fold starts a sixteenth of a cell past the middle grid row, so for gap < 7 h / 16 no vertex lies on the fold.  -> (x [nv][3],
    tris): sym_plane's vertex order and sheet_tris' topology, unchanged.  Only + - * / on float64 and exact constants, so every host
    gives the same bits."""
    x, tris = sym_plane(w, l)
    nv = (w + 1) * (l + 1)
    jj = np.concatenate([np.repeat(np.arange(l + 1, dtype=np.float64), w + 1), np.repeat(np.arange(l, dtype=np.float64) + 0.5, w)])
    assert len(jj) == len(x) and nv + w * l == len(x)
    s = jj / w
    a = (l // 2 + 0.0625) / w
    g = float(gap)
    lower, fold = s <= a, (s > a) & (s <= a + g)
    x[:, 1] = np.where(lower, 0.0, np.where(fold, s - a, g))
    x[:, 2] = np.where(lower, s, np.where(fold, a, a - ((s - a) - g)))
    return x, tris


def bend_hinges(tris):
    """One hinge (i0, i1, i2, i3) per interior edge: i2,i3 the shared edge,
    i0/i1 the opposite vertices (BendForce rows are x0-x2, x3-x2, x1-x2;
    reference deps/admm-elastic-sca/src/system/BendForce.cpp:58-118)."""
    edge = {}
    hinges = []
    for t, (a, b, c) in enumerate(tris):
        for (p, q, o) in ((a, b, c), (b, c, a), (c, a, b)):
            key = (min(p, q), max(p, q))
            if key in edge:
                o2 = edge[key]
                hinges.append((o2, o, key[0], key[1]))
            else:
                edge[key] = o
    return np.array(hinges, dtype=np.int32).reshape(-1, 4)
