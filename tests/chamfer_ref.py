"""numpy-only float64 restatement of the reference's evaluation/dtu_eval.py (line numbers in brackets): what
uforecon_amd/csrc/chamfer.hip and uforecon_amd/dtu_eval.py are tested against, itself pinned to recorded outputs of the
reference script (tests/golden/chamfer_*.npz, made by tests/golden/make_golden_chamfer.py).

No sklearn / scipy / open3d: neighbours come from brute force (small sets) or a numpy grid (large ones); the thinning is
the reference's sequential loop as written."""
import numpy as np


# ------------------------------------------------------------------ [68-91] mesh -> point cloud
def triangle_setup(vertices, triangles, density):
    """[70-85]: v1, v2, the first corners, n1, n2 of the triangles with a non-zero area, and which triangles those are."""
    tri_vert = vertices[triangles]
    v1 = tri_vert[:, 1] - tri_vert[:, 0]
    v2 = tri_vert[:, 2] - tri_vert[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    non_zero_area = (area2 > 0)[:, 0]
    l1, l2, area2, v1, v2, tri_vert = [arr[non_zero_area] for arr in [l1, l2, area2, v1, v2, tri_vert]]
    thr = density * np.sqrt(l1 * l2 / area2)
    n1 = np.floor(l1 / thr)
    n2 = np.floor(l2 / thr)
    return v1, v2, tri_vert[:, 0], n1[:, 0], n2[:, 0], non_zero_area


def lattice(n1, n2):
    """[12-19] sample_single_tri's (a, b) pairs for one (n1, n2)."""
    c = np.mgrid[:n1 + 1, :n2 + 1]
    c += 0.5
    c[0] /= max(n1, 1e-7)
    c[1] /= max(n2, 1e-7)
    c = np.transpose(c, (1, 2, 0))
    return c[c.sum(axis=-1) < 1]


def sample_mesh(vertices, triangles, density, return_counts=False):
    """[68-91]: the vertices followed by every triangle's samples in (triangle, i, j) order.  The lattice depends only on
    (n1, n2), so triangles are handled in groups that share it; within a group the arithmetic is sample_single_tri's."""
    vertices = np.asarray(vertices, np.float64)
    v1, v2, p0, n1, n2, nz = triangle_setup(vertices, np.asarray(triangles), density)
    pairs, inv = np.unique(np.stack([n1, n2], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    lat = [lattice(a, b) for a, b in pairs]
    counts = np.array([len(k) for k in lat], np.int64)[inv]
    off = np.concatenate([[0], np.cumsum(counts)])
    new_pts = np.empty((off[-1], 3), np.float64)
    for g, k in enumerate(lat):
        if len(k) == 0:
            continue
        idx = np.nonzero(inv == g)[0]
        q = v1[idx, None, :] * k[None, :, :1] + v2[idx, None, :] * k[None, :, 1:] + p0[idx, None, :]     # [20]
        rows = off[idx][:, None] + np.arange(len(k))[None, :]
        new_pts[rows.reshape(-1)] = q.reshape(-1, 3)
    out = np.concatenate([vertices, new_pts], axis=0)
    if return_counts:
        per_tri = np.zeros(len(triangles), np.int64)
        per_tri[nz] = counts
        return out, dict(n1=n1, n2=n2, non_zero_area=nz, per_triangle=per_tri)
    return out


# ------------------------------------------------------------------ [105-115] thinning
def _d2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius_neighbours_brute(points, r, chunk=512):
    """what radius_neighbors returns (distance <= r, the point itself included), by brute force"""
    out = []
    for s in range(0, len(points), chunk):
        m = _d2(points[s:s + chunk, None, :], points[None, :, :]) <= r * r
        out.extend(np.nonzero(row)[0] for row in m)
    return out


def thin_sequential(points, r):
    """[107-114] with the neighbour lists by brute force: the loop as the reference writes it."""
    rnn_idxs = radius_neighbours_brute(points, r)
    mask = np.ones(points.shape[0], dtype=np.bool_)
    for curr, idxs in enumerate(rnn_idxs):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    return mask


def _cells(points, origin, cell):
    c = np.floor((points - origin) / cell).astype(np.int64) + 1
    dims = c.max(0) + 2
    return c, dims


def earlier_neighbours_grid(points, r):
    """CSR lists (start, idx) of the points j < i within r of point i, from a uniform grid of cell size r * (1 + 1e-9)."""
    n = len(points)
    cell = r * (1 + 1e-9) if r > 0 else 1.0
    c, dims = _cells(points, points.min(0), cell)
    key = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ii, jj = [], []
    me = np.arange(n)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            lo_key = ((c[:, 0] + dx) * dims[1] + c[:, 1] + dy) * dims[2] + c[:, 2] - 1      # the three z cells are one key run
            s = np.searchsorted(skey, lo_key, "left")
            e = np.searchsorted(skey, lo_key + 2, "right")
            cnt = e - s
            for k in range(int(cnt.max()) if n else 0):
                v = np.nonzero(cnt > k)[0]
                j = order[s[v] + k]
                near = (j < me[v]) & (_d2(points[v], points[j]) <= r * r)
                ii.append(me[v][near])
                jj.append(j[near])
    ii = np.concatenate(ii) if ii else np.zeros(0, np.int64)
    jj = np.concatenate(jj) if jj else np.zeros(0, np.int64)
    o = np.argsort(ii, kind="stable")
    ii, jj = ii[o], jj[o]
    start = np.searchsorted(ii, np.arange(n + 1), "left")
    return start, jj


def thin_grid(points, r):
    """The same mask as thin_sequential for large clouds: a point is kept iff none of its earlier neighbours is kept (what the
    reference's loop computes: a kept point clears all its neighbours, so a later point survives iff no earlier kept point is
    within r)."""
    start, nbr = earlier_neighbours_grid(points, r)
    keep = np.ones(len(points), np.bool_)
    nonempty = np.nonzero(start[1:] > start[:-1])[0]
    for i in nonempty:
        if keep[nbr[start[i]:start[i + 1]]].any():
            keep[i] = False
    return keep


# ------------------------------------------------------------------ [117-131] observation mask
def observation_filter(data_down, ObsMask, BB, Res, patch):
    """[121-131]: (inbound over data_down, grid_inbound over data_in, in_obs over data_in[grid_inbound])."""
    BB = BB.astype(np.float32)
    inbound = ((data_down >= BB[:1] - patch) & (data_down < BB[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = data_down[inbound]
    data_grid = np.around((data_in - BB[:1]) / Res).astype(np.int32)
    grid_inbound = ((data_grid >= 0) & (data_grid < np.expand_dims(ObsMask.shape, 0))).sum(axis=-1) == 3
    data_grid_in = data_grid[grid_inbound]
    in_obs = ObsMask[data_grid_in[:, 0], data_grid_in[:, 1], data_grid_in[:, 2]].astype(np.bool_)
    return inbound, grid_inbound, in_obs


# ------------------------------------------------------------------ [139-155] nearest neighbours
def nn_brute(query, ref, chunk=256):
    """exact nearest-neighbour distances, sqrt((dx*dx + dy*dy) + dz*dz), by brute force"""
    out = np.empty(len(query), np.float64)
    for s in range(0, len(query), chunk):
        out[s:s + chunk] = np.sqrt(_d2(query[s:s + chunk, None, :], ref[None, :, :]).min(1))
    return out


def nn_grid(query, ref, max_dist):
    """Nearest-neighbour distances wherever they are < max_dist, +inf elsewhere: a grid of cell size max_dist over the
    reference set, 27 cells per query (a point outside them is at least one cell away)."""
    origin = ref.min(0)
    cr, dims = _cells(ref, origin, max_dist)
    cq = np.floor((query - origin) / max_dist).astype(np.int64) + 1
    inside = ((cq >= 0) & (cq < dims)).all(1)            # a query outside the padded grid has nothing within max_dist
    key = (cr[:, 0] * dims[1] + cr[:, 1]) * dims[2] + cr[:, 2]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    best = np.full(len(query), np.inf)
    qi = np.nonzero(inside)[0]
    q, c = query[qi], cq[qi]
    b = np.full(len(qi), np.inf)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            x, y = c[:, 0] + dx, c[:, 1] + dy
            ok = (x >= 0) & (x < dims[0]) & (y >= 0) & (y < dims[1])
            z0, z1 = np.maximum(c[:, 2] - 1, 0), np.minimum(c[:, 2] + 1, dims[2] - 1)
            s = np.searchsorted(skey, (x * dims[1] + y) * dims[2] + z0, "left")
            e = np.searchsorted(skey, (x * dims[1] + y) * dims[2] + z1, "right")
            cnt = np.where(ok, e - s, 0)
            for k in range(int(cnt.max()) if len(qi) else 0):
                v = np.nonzero(cnt > k)[0]
                b[v] = np.minimum(b[v], _d2(q[v], ref[order[s[v] + k]]))
    best[qi] = np.sqrt(b)
    best[~(best < max_dist)] = np.inf
    return best


# ------------------------------------------------------------------ the whole script for one scan
def chamfer(data, gt_points, ObsMask, BB, Res, plane, density=0.2, patch=60, max_dist=20, seed=0, nn=nn_brute,
            thin=thin_sequential):
    """dtu_eval.py's loop body.  ``data``: (vertices, triangles) for --mode mesh, a point array for --mode pcd.  The
    shuffle [101-103] is default_rng(seed).permutation(N) applied as a gather (equal to a seeded generator's shuffle)."""
    r = {}
    if isinstance(data, tuple):
        data_pcd = sample_mesh(np.asarray(data[0], np.float64), data[1], density)
    else:
        data_pcd = np.asarray(data, np.float64)
    r["data_pcd_unshuffled"] = data_pcd
    data_pcd = data_pcd[np.random.default_rng(seed).permutation(len(data_pcd))]
    mask = thin(data_pcd, density)
    data_down = data_pcd[mask]
    inbound, grid_inbound, in_obs = observation_filter(data_down, ObsMask, BB, Res, patch)
    data_in = data_down[inbound]
    data_in_obs = data_in[grid_inbound][in_obs]
    stl = np.asarray(gt_points, np.float64)
    dist_d2s = nn(data_in_obs, stl)
    mean_d2s = dist_d2s[dist_d2s < max_dist].mean()
    stl_hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
    above = (np.asarray(plane, np.float64).reshape((1, 4)) * stl_hom).sum(-1) > 0
    stl_above = stl[above]
    dist_s2d = nn(stl_above, data_in)
    mean_s2d = dist_s2d[dist_s2d < max_dist].mean()
    r.update(data_pcd=data_pcd, thin_mask=mask, inbound=inbound, grid_inbound=grid_inbound, in_obs=in_obs, above=above,
             data_in=data_in, data_in_obs=data_in_obs, stl_above=stl_above, dist_d2s=dist_d2s, dist_s2d=dist_s2d,
             d2s=float(mean_d2s), s2d=float(mean_s2d), overall=float((mean_d2s + mean_s2d) / 2),
             counts=dict(sampled=len(data_pcd), thinned=int(mask.sum()), in_box=int(inbound.sum()),
                         in_grid=int(grid_inbound.sum()), in_obs=int(in_obs.sum()), gt=len(stl), gt_above=int(above.sum())))
    return r
