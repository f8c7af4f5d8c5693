"""The numpy statement of the point-cloud filters (include/ufr.h, "point-cloud filtering"; uforecon_amd/pcd_filter.py): brute
force where the kernels walk an octree, the same fp64 expressions and the same summation orders, so that indices, masks and
most values can be compared bit for bit.  The rules follow the public descriptions of PCL's and Open3D's filters; neither
library was compared against.  Sizes are test sizes: the k-NN forms the whole (nq, nr) distance matrix."""
from __future__ import annotations

import numpy as np

KNN_MAX_K = 32
KEY_BITS = 21


# ------------------------------------------------------------------ test clouds
def sphere_cloud(n=2000, n_far=12, noise=0.002, seed=0):
    """n points on the unit sphere with radial noise, then n_far points at radius 1.6 .. 2.2: (n + n_far, 3) float64."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n + n_far, 3))
    d /= np.sqrt((d * d).sum(1))[:, None]
    r = np.concatenate([1.0 + noise * rng.standard_normal(n), rng.uniform(1.6, 2.2, n_far)])
    return np.ascontiguousarray(d * r[:, None])


# ------------------------------------------------------------------ k nearest neighbours
def dist2(query, ref):
    """(nq, nr) float64: (dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own."""
    q = np.asarray(query, np.float64)[:, None, :]
    r = np.asarray(ref, np.float64)[None, :, :]
    dx, dy, dz = q[..., 0] - r[..., 0], q[..., 1] - r[..., 1], q[..., 2] - r[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def knn(query, ref, k, max_dist=np.inf, exclude_self=False):
    """idx (nq, k) int32 and dist (nq, k) float64: per query the k smallest keys (d2, index) with d2 <= max_dist^2, ascending;
    empty slots -1 and inf; a query that is not finite gets only empty slots; exclude_self drops candidate i of query i."""
    query, ref = np.asarray(query, np.float64), np.asarray(ref, np.float64)
    nq, nr = len(query), len(ref)
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float64)
    if nq == 0 or nr == 0:
        return idx, dist
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = dist2(query, ref)
        md2 = np.float64(max_dist) * np.float64(max_dist)
        ok = d2 <= md2
    ok &= np.isfinite(query).all(1)[:, None]
    if exclude_self:
        assert nq == nr
        ok[np.arange(nq), np.arange(nq)] = False
    index = np.arange(nr)
    for i in range(nq):
        cand = index[ok[i]]
        order = cand[np.lexsort((cand, d2[i, cand]))][:k]          # by d2, ties to the lower index
        idx[i, :len(order)] = order
        dist[i, :len(order)] = np.sqrt(d2[i, order])
    return idx, dist


# ------------------------------------------------------------------ outlier filters
def mean_neighbour_distance(idx, dist):
    """Per row the left-to-right sum of the non-empty slots' distances divided by their number; inf for an empty row."""
    s = np.zeros(len(idx), np.float64)
    for j in range(idx.shape[1]):
        s = s + np.where(idx[:, j] >= 0, dist[:, j], 0.0)
    m = (idx >= 0).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > 0, s / m, np.inf)


def statistical(points, nb_neighbors=20, std_ratio=2.0):
    """keep, avg, threshold: avg = the mean distance to the nb_neighbors nearest other points; threshold = mean + std_ratio *
    population standard deviation over the finite avg; keep = avg <= threshold."""
    idx, dist = knn(points, points, nb_neighbors, exclude_self=True)
    avg = mean_neighbour_distance(idx, dist)
    fin = avg[np.isfinite(avg)]
    threshold = float(fin.mean() + std_ratio * fin.std()) if len(fin) else float("inf")
    return avg <= threshold, avg, threshold


def radius(points, nb_points, radius):
    """keep: at least nb_points other points lie within radius (inclusive)."""
    idx, _ = knn(points, points, nb_points, max_dist=radius, exclude_self=True)
    return (idx >= 0).sum(1) >= nb_points


# ------------------------------------------------------------------ normals
def covariance(points, idx):
    """m (n,), centroid (n,3) and covariance (n,3,3) of every row's non-empty slots, summed in slot order."""
    points = np.asarray(points, np.float64)
    n = len(points)
    ok = (idx >= 0) & (idx < n)
    m = ok.sum(1)
    safe = np.where(ok, idx, 0)
    s = np.zeros((n, 3))
    for j in range(idx.shape[1]):
        s = s + np.where(ok[:, j, None], points[safe[:, j]], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = s / m[:, None].astype(np.float64)
    six = np.zeros((n, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(idx.shape[1]):
        with np.errstate(invalid="ignore"):
            d = points[safe[:, j]] - c
        for t, (a, b) in enumerate(pairs):
            six[:, t] = six[:, t] + np.where(ok[:, j], d[:, a] * d[:, b], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        six = six / m[:, None].astype(np.float64)
    cov = np.empty((n, 3, 3))
    for t, (a, b) in enumerate(pairs):
        cov[:, a, b] = six[:, t]
        cov[:, b, a] = six[:, t]
    return m, c, cov


def orient(normals, points, viewpoints=None):
    """The sign rule: towards the viewpoint with the largest |cos| (ties to the lowest), or, without viewpoints, the
    component of largest magnitude positive (ties to the lowest axis).  Also returns that largest |cos| (None without)."""
    n = np.array(normals, np.float64)
    if viewpoints is not None and len(viewpoints):
        v = np.asarray(viewpoints, np.float64)[None, :, :] - np.asarray(points, np.float64)[:, None, :]
        dot = (n[:, None, 0] * v[..., 0] + n[:, None, 1] * v[..., 1]) + n[:, None, 2] * v[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = np.abs(dot) / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        cos = np.where(np.isnan(cos), -1.0, cos)
        j = cos.argmax(1)                                             # the first of equal maxima
        flip = dot[np.arange(len(n)), j] < 0
        best = cos.max(1)
    else:
        ax = np.abs(n).argmax(1)
        flip = n[np.arange(len(n)), ax] < 0
        best = None
    n[flip] = -n[flip]
    return n, best


def normals(points, idx, viewpoints=None):
    """normal, curvature, valid, and (cov, eigenvalues (n,3) ascending, best |cos|) for the tests' own checks."""
    points = np.asarray(points, np.float64)
    m, _, cov = covariance(points, idx)
    valid = m >= 3
    w, v = np.linalg.eigh(np.where(valid[:, None, None], cov, np.eye(3)))
    nrm, best = orient(v[:, :, 0], points, viewpoints)
    tr = (w[:, 0] + w[:, 1]) + w[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        curv = np.where(tr != 0, w[:, 0] / tr, 0.0)
    nrm[~valid] = 0.0
    curv[~valid] = 0.0
    return nrm, curv, valid.astype(np.uint8), (cov, w, best)


# ------------------------------------------------------------------ voxel mean
def _spread3(x):
    x = x.astype(np.uint64) & np.uint64(0x1FFFFF)
    for s, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                    (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(s))) & np.uint64(mask)
    return x


def cell_keys(points, origin, cell):
    """The int64 Morton key (x highest of every bit triple) of floor((p - origin) / cell), clamped to 0 .. 2^21 - 1."""
    t = np.floor((np.asarray(points, np.float64) - np.asarray(origin, np.float64)) / np.float64(cell))
    c = np.clip(np.nan_to_num(t, nan=0.0), 0, 2 ** KEY_BITS - 1).astype(np.int64)
    return (_spread3(c[:, 0]) << np.uint64(2) | _spread3(c[:, 1]) << np.uint64(1) | _spread3(c[:, 2])).astype(np.int64)


def voxel_mean(points, voxel, colors=None, normals=None):
    """points (m,3), colors (m,3) uint8 or None, normals (m,3) or None, count (m,) int32: one row per occupied voxel of the
    grid with origin min_bound - voxel / 2, in Morton-key order; every voxel summed in ascending index order."""
    points = np.asarray(points, np.float64)
    origin = points.min(0) - np.float64(voxel) / 2
    cells = np.floor((points.max(0) - origin) / np.float64(voxel)) + 1
    if cells.max() > 2 ** KEY_BITS - 4:
        raise ValueError(f"voxel_mean: {int(cells.max())} cells on an axis")
    keys = cell_keys(points, origin, voxel)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    heads = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    ends = np.concatenate([heads[1:], [len(ks)]])
    out_p = np.empty((len(heads), 3))
    out_c = None if colors is None else np.empty((len(heads), 3), np.uint8)
    out_n = None if normals is None else np.empty((len(heads), 3))
    count = (ends - heads).astype(np.int32)
    for r, (a, b) in enumerate(zip(heads, ends)):
        s = np.zeros(3)
        sn = np.zeros(3)
        sc = np.zeros(3, np.int64)
        for j in order[a:b]:
            s = s + points[j]
            if colors is not None:
                sc = sc + colors[j].astype(np.int64)
            if normals is not None:
                sn = sn + normals[j]
        c = int(b - a)
        out_p[r] = s / np.float64(c)
        if colors is not None:
            out_c[r] = (2 * sc + c) // (2 * c)
        if normals is not None:
            ln = np.sqrt((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2])
            out_n[r] = sn / ln if ln > 0 else 0.0
    return out_p, out_c, out_n, count
