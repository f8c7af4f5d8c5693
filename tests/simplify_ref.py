"""The numpy statement of mesh simplification (include/ufr.h, "mesh simplification"; uforecon_amd/csrc/mesh_simplify.hip): vertex
clustering with quadric placement, every product and sum a statement of its own, every sum left to right (``np.add.at`` adds
its rows one after the other, in the order given), so that the device's bits can be asked for.  Also the fixtures both test
files share: the tessellated cube, the two-layer patch, the slab, the soup."""
import numpy as np

import pcd_ref
from color_mesh_ref import icosphere  # noqa: F401  (a fixture of both test files)

NONE = np.int64(2 ** 63 - 1)
MAX_CELLS = 2 ** 21 - 4
REG = np.float64(2.0 ** -10)
BISECTION_STEPS = 32


# ------------------------------------------------------------------ fixtures
def cube(n=9):
    """the surface of the unit cube, n x n vertices per side (shared along the edges), outward winding"""
    ids, verts, faces = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append([c / (n - 1) for c in p])
        return ids[p]

    for axis in range(3):
        for side in (0, n - 1):
            for i in range(n - 1):
                for j in range(n - 1):
                    def at(a, b):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, a, b
                        return vid(tuple(p))
                    q = [at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)]      # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.asarray(verts, np.float64), np.asarray(faces, np.int32)


def grid_patch(n, size=1.0, z=0.0, flip=False):
    xs = np.linspace(0.0, size, n)
    v = np.array([(x, y, z) for y in xs for x in xs], np.float64)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [(a, a + 1, a + n), (a + 1, a + n + 1, a + n)]
    f = np.asarray(f, np.int32)
    return v, (f[:, ::-1].copy() if flip else f)


def two_layer_patch(n=13, cell=0.25):
    """a grid patch and a copy of it 0.01 cell higher: the copy's faces fall on the same cluster triples"""
    v0, f0 = grid_patch(n)
    v1, f1 = grid_patch(n, z=0.01 * cell)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


def slab(n=13, thickness=0.02):
    """a closed slab: the top sheet, the mirrored bottom sheet and the four walls"""
    vt, ft = grid_patch(n, z=thickness)
    vb, fb = grid_patch(n, z=0.0, flip=True)
    walls = []
    rim = ([(i, i + 1) for i in range(n - 1)] + [(n * (n - 1) + i + 1, n * (n - 1) + i) for i in range(n - 1)]
           + [((j + 1) * n, j * n) for j in range(n - 1)] + [(j * n + n - 1, (j + 1) * n + n - 1) for j in range(n - 1)])
    for a, b in rim:
        walls += [(a, a + n * n, b), (b, a + n * n, b + n * n)]
    return np.concatenate([vt, vb]), np.concatenate([ft, fb + n * n, np.asarray(walls, np.int32)]).astype(np.int32)


def soup(V, F, seed=0):
    """V random vertices of the unit cube and F random triangles over them (corners may repeat)"""
    rng = np.random.default_rng(seed)
    return rng.random((V, 3)), rng.integers(0, V, (F, 3)).astype(np.int32)


def colors_of(V, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (V, 3)).astype(np.uint8)


# ------------------------------------------------------------------ the rule
def _compact3(x):
    x = x.astype(np.uint64) & np.uint64(0x1249249249249249)
    for s, mask in ((2, 0x10C30C30C30C30C3), (4, 0x100F00F00F00F00F), (8, 0x1F0000FF0000FF), (16, 0x1F00000000FFFF), (32, 0x1FFFFF)):
        x = (x | (x >> np.uint64(s))) & np.uint64(mask)
    return x


def sorted_keys(verts, cell):
    """(origin, keys, stable order) of the clustering grid: the setup of pcd_ref.voxel_mean"""
    cell = np.float64(cell)
    origin = verts.min(0) - cell / 2
    cells = np.floor((verts.max(0) - origin) / cell) + 1
    if not cells.max() <= MAX_CELLS:
        raise ValueError(f"simplify: {cells.max():.0f} cells on an axis")
    keys = pcd_ref.cell_keys(verts, origin, cell)
    return origin, keys, np.argsort(keys, kind="stable")


def count_cells(verts, cell):
    return len(np.unique(sorted_keys(verts, cell)[1]))


def target_cell(verts, N):
    e = verts.max(0) - verts.min(0)
    lo = e.max() * np.float64(2.0 ** -20)
    hi = np.float64(2.0) * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    for _ in range(BISECTION_STEPS):
        mid = np.sqrt(lo * hi)
        if count_cells(verts, mid) <= N:
            hi = mid
        else:
            lo = mid
    return float(hi)


def cell_centres(ckey, origin, cell):
    k = ckey.astype(np.uint64)
    ijk = np.stack([_compact3(k >> np.uint64(2)), _compact3(k >> np.uint64(1)), _compact3(k)], 1).astype(np.float64)
    return origin + (ijk + 0.5) * np.float64(cell)


def face_quadrics(verts, faces, cluster, centres):
    """quadrics (C,10) and n_faces (C,): every cluster's sums over its faces in ascending face index"""
    C = len(centres)
    F = len(faces)
    c = cluster[faces]
    f = np.arange(F)
    rows = [(c[:, 0], f)]
    s1 = c[:, 1] != c[:, 0]
    rows.append((c[s1, 1], f[s1]))
    s2 = (c[:, 2] != c[:, 0]) & (c[:, 2] != c[:, 1])
    rows.append((c[s2, 2], f[s2]))
    cl = np.concatenate([r[0] for r in rows]).astype(np.int64)
    fi = np.concatenate([r[1] for r in rows]).astype(np.int64)
    order = np.argsort(cl << np.int64(32) | fi, kind="stable")
    cl, fi = cl[order], fi[order]
    pa, pb, pc = verts[faces[fi, 0]], verts[faces[fi, 1]], verts[faces[fi, 2]]
    u, v = pb - pa, pc - pa
    n0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    n1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    n2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    r = pa - centres[cl]
    d = -((n0 * r[:, 0] + n1 * r[:, 1]) + n2 * r[:, 2])
    terms = np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, n0 * d, n1 * d, n2 * d, d * d], 1)
    Q = np.zeros((C, 10))
    np.add.at(Q, cl, terms)
    return Q, np.bincount(cl, minlength=C).astype(np.int32)


def _error(A, b, c, y):
    g0 = (A[0] * y[0] + A[1] * y[1]) + A[2] * y[2]
    g1 = (A[1] * y[0] + A[3] * y[1]) + A[4] * y[2]
    g2 = (A[2] * y[0] + A[4] * y[1]) + A[5] * y[2]
    quad = (y[0] * g0 + y[1] * g1) + y[2] * g2
    lin = (b[0] * y[0] + b[1] * y[1]) + b[2] * y[2]
    return (quad + 2.0 * lin) + c


def place(Q, n_faces, mean, centres, cell, placement):
    """position (C,3), placed (C,) uint8"""
    if placement == "mean":
        return mean.copy(), np.zeros(len(mean), np.uint8)
    assert placement == "quadric"
    q = Q.T
    xb = (mean - centres).T
    w = REG * ((q[0] + q[3]) + q[5])
    A = [q[0] + w, q[1], q[2], q[3] + w, q[4], q[5] + w]
    b = [q[6] - w * xb[0], q[7] - w * xb[1], q[8] - w * xb[2]]
    c = q[9] + w * ((xb[0] * xb[0] + xb[1] * xb[1]) + xb[2] * xb[2])
    with np.errstate(all="ignore"):
        C00 = A[3] * A[5] - A[4] * A[4]
        C01 = A[2] * A[4] - A[1] * A[5]
        C02 = A[1] * A[4] - A[2] * A[3]
        C11 = A[0] * A[5] - A[2] * A[2]
        C12 = A[1] * A[2] - A[0] * A[4]
        C22 = A[0] * A[3] - A[1] * A[1]
        det = (A[0] * C00 + A[1] * C01) + A[2] * C02
        r = [-b[0], -b[1], -b[2]]
        x = [((C00 * r[0] + C01 * r[1]) + C02 * r[2]) / det,
             ((C01 * r[0] + C11 * r[1]) + C12 * r[2]) / det,
             ((C02 * r[0] + C12 * r[1]) + C22 * r[2]) / det]
        half = np.float64(0.5) * np.float64(cell)
        take = (n_faces > 0) & np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])
        take &= (np.abs(x[0]) <= half) & (np.abs(x[1]) <= half) & (np.abs(x[2]) <= half)
        take &= _error(A, b, c, x) <= _error(A, b, c, xb)
        pos = centres + np.stack(x, 1)
    return np.where(take[:, None], pos, mean), take.astype(np.uint8)


def simplify(verts, faces, colors=None, cell=None, target_vertices=None, placement="quadric"):
    """The outputs of ops.mesh_simplify as numpy arrays, in a dict of the same keys."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(verts), len(faces)
    assert (cell is None) != (target_vertices is None)
    if target_vertices is not None and V <= target_vertices:
        return dict(verts=verts.copy(), faces=faces.copy(), colors=None if colors is None else colors.copy(),
                    vertex_map=np.arange(V, dtype=np.int32), face_map=np.arange(F, dtype=np.int32), placed=np.zeros(V, np.uint8),
                    count=np.ones(V, np.int32), cell=0.0, clusters=V, collapsed_faces=0, duplicate_faces=0)
    cell = float(cell) if cell is not None else target_cell(verts, target_vertices)
    if V == 0 or F == 0:
        return dict(verts=np.zeros((0, 3)), faces=np.zeros((0, 3), np.int32), colors=None if colors is None else np.zeros((0, 3), np.uint8),
                    vertex_map=np.full(V, -1, np.int32), face_map=np.zeros(0, np.int32), placed=np.zeros(0, np.uint8),
                    count=np.zeros(0, np.int32), cell=cell, clusters=0, collapsed_faces=F, duplicate_faces=0)
    origin, keys, order = sorted_keys(verts, cell)
    ks = keys[order]
    head = np.concatenate([[True], ks[1:] != ks[:-1]])
    cluster = np.empty(V, np.int64)
    cluster[order] = np.cumsum(head) - 1
    ckey = ks[head]
    C = len(ckey)
    # count, mean (left to right in ascending vertex index), rounded mean colour: ufr_points_voxel_mean
    count = np.bincount(cluster, minlength=C).astype(np.int32)
    s = np.zeros((C, 3))
    np.add.at(s, cluster[order], verts[order])
    mean = s / count[:, None].astype(np.float64)
    ccol = None
    if colors is not None:
        sc = np.zeros((C, 3), np.int64)
        np.add.at(sc, cluster, colors.astype(np.int64))
        ccol = ((2 * sc + count[:, None]) // (2 * count[:, None].astype(np.int64))).astype(np.uint8)
    centres = cell_centres(ckey, origin, cell)
    Q, n_faces = face_quadrics(verts, faces, cluster, centres)
    position, placed = place(Q, n_faces, mean, centres, cell, placement)
    # faces: remap, drop the collapsed, rotate, keep the lowest input index of every rotated triple
    c = cluster[faces]
    ok = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    first = np.argmin(c, 1)
    tri = np.stack([c[np.arange(F), (first + e) % 3] for e in range(3)], 1)
    key_a = np.where(ok, tri[:, 0], NONE)
    key_bc = np.where(ok, tri[:, 1] << np.int64(32) | tri[:, 2], NONE)
    o1 = np.argsort(key_bc, kind="stable")
    o2 = np.argsort(key_a[o1], kind="stable")
    o = o1[o2]
    a_s, bc_s = key_a[o], key_bc[o]
    run_head = np.concatenate([[True], (a_s[1:] != a_s[:-1]) | (bc_s[1:] != bc_s[:-1])]) & (a_s != NONE)
    keep = np.zeros(F, bool)
    keep[o] = run_head
    face_map = np.flatnonzero(keep).astype(np.int32)
    out_faces = tri[keep]
    referenced = np.zeros(C, bool)
    referenced[out_faces.reshape(-1)] = True
    cluster_vertex = np.where(referenced, np.cumsum(referenced) - 1, -1)
    return dict(verts=position[referenced], faces=cluster_vertex[out_faces].astype(np.int32).reshape(-1, 3),
                colors=None if ccol is None else ccol[referenced], vertex_map=cluster_vertex[cluster].astype(np.int32),
                face_map=face_map, placed=placed[referenced], count=count[referenced], cell=cell, clusters=C,
                collapsed_faces=int((~ok).sum()), duplicate_faces=int(ok.sum() - keep.sum()),
                centres=centres[referenced])
