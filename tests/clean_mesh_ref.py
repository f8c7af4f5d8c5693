"""numpy float64 restatement of the four stages of DTU mesh cleaning (include/ufr.h, "DTU mesh cleaning"; the reference's
evaluation/clean_mesh.py).  Slow and plain on purpose: the first hit is brute force over every (ray, face) pair, the components
come from scipy.sparse.csgraph.  The kernels of csrc/mesh_clean.hip are pinned to this file, and this file to the recorded
outputs of the reference's own functions (tests/golden/clean_mesh_*.npz).

A pixel is *close* (``first_hit(..., return_close=True)``) when, by the margins computed here,
  * some face whose plane the ray crosses at t > 0 has every barycentric coordinate >= -1e-6 and one <= 1e-6 (the ray passes
    within 1e-6 of an edge or vertex, of its hit or of a near-hit), or
  * its two nearest hits differ by less than 1e-6 relative in t.
"""
import numpy as np

BARY_MARGIN = 1e-6
T_MARGIN = 1e-6


# ------------------------------------------------------------------ stage 1: mask dilation
def half_widths(k):
    """rows of cv.getStructuringElement(MORPH_ELLIPSE, (k, k)), k odd, as half-widths"""
    assert k >= 1 and k % 2 == 1
    r = k // 2
    if r == 0:
        return [0]
    return [int(np.rint(r * np.sqrt((r * r - dy * dy) / (r * r)))) for dy in range(-r, r + 1)]   # np.rint: half to even


def ellipse(k):
    hw = half_widths(k)
    r = k // 2
    el = np.zeros((k, k), np.uint8)
    for i, w in enumerate(hw):
        el[i, r - w:r + w + 1] = 1
    return el


def dilate(img, k):
    """cv.dilate(img, ellipse(k)) of a (H,W) uint8 image; pixels outside the image are ignored"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    r = k // 2
    pad = np.zeros((H + 2 * r, W + 2 * r), np.uint8)      # 0 is the neutral element of a uint8 maximum
    pad[r:r + H, r:r + W] = img
    out = np.zeros_like(img)
    for i, w in enumerate(half_widths(k)):
        for dx in range(-w, w + 1):
            out = np.maximum(out, pad[i:i + H, r + dx:r + dx + W])
    return out


def dilated_mask(img, k=11, threshold=128):
    return dilate(img, k) > threshold


# ------------------------------------------------------------------ stage 2: vertex votes
def projection(K, E):
    """read_cam_file: P = K4 @ E in float32"""
    K4 = np.float32(np.diag([1, 1, 1, 1]))
    K4[:3, :3] = np.asarray(K, np.float32)
    return K4 @ np.asarray(E, np.float32)


def vertex_votes(verts, Ps, masks):
    """votes (V,) int32; masks: (NV,H,W) bool, the dilated masks"""
    verts = np.asarray(verts, np.float64)
    votes = np.zeros(len(verts), np.int32)
    for P, m in zip(Ps, masks):
        P = np.asarray(P, np.float32).astype(np.float64)
        H, W = m.shape
        x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
        with np.errstate(all="ignore"):
            q = [((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3] for i in range(3)]
            ok = (q[2] / q[2]) == 1.0
            rx, ry = np.rint(q[0] / q[2]), np.rint(q[1] / q[2])
            ok &= (rx >= -1) & (rx <= W - 1) & (ry >= -1) & (ry <= H - 1)
        px = np.where(ok, rx, 0).astype(np.int64)
        py = np.where(ok, ry, 0).astype(np.int64)
        border = (px == -1) | (py == -1)
        inside = np.asarray(m, bool)[py.clip(0), px.clip(0)]
        votes += (ok & (border | inside)).astype(np.int32)
    return votes


def keep_by_votes(verts, faces, votes, minimal_vis=1):
    """(stage-2 vertices, faces, vertex keep mask): compaction in the original order"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = votes > minimal_vis
    index = np.cumsum(keep) - 1
    fkeep = keep[faces[:, 0]] & keep[faces[:, 1]] & keep[faces[:, 2]] if len(faces) else np.zeros(0, bool)
    return np.asarray(verts)[keep], index[faces[fkeep]].astype(np.int32), keep


# ------------------------------------------------------------------ stage 3: first-hit faces
def camera(K, E):
    """(K / K[2,2] float64 3x3, c2w = inv(E) in float64, normalised by its [3,3] (1 unless E was scaled as a whole), narrowed
    to float32 4x4)"""
    K = np.asarray(K, np.float32).astype(np.float64)
    c2w = np.linalg.inv(np.asarray(E, np.float32).astype(np.float64))
    return K / K[2, 2], (c2w / c2w[3, 3]).astype(np.float32)


def k_inverse(K):
    """torch.inverse of the float32 intrinsics, as gen_rays_from_single_image forms it"""
    import torch

    return torch.inverse(torch.from_numpy(np.asarray(K, np.float64)).float()).numpy()


def rays(k_inv, c2w, H, W):
    """(origin (3,), directions (H,W,3)) in float32, every product summed left to right"""
    ki, cw = np.asarray(k_inv, np.float32), np.asarray(c2w, np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    one = np.float32(1)
    p = [(ki[i, 0] * xs + ki[i, 1] * ys) + ki[i, 2] * one for i in range(3)]
    n = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
    v = [c / n for c in p]
    d = np.stack([(cw[i, 0] * v[0] + cw[i, 1] * v[1]) + cw[i, 2] * v[2] for i in range(3)], -1)
    assert d.dtype == np.float32
    return cw[:3, 3].copy(), d


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def _cross_ordered(u, iu, v, iv):
    """u x v, formed for the lower vertex index first and negated otherwise"""
    fwd = (iu <= iv)[:, None]
    return np.where(fwd, _cross(u, v), -_cross(v, u))


def _dot(d, c):
    """(R,3) . (F,3) -> (R,F), summed left to right"""
    return (d[:, None, 0] * c[None, :, 0] + d[:, None, 1] * c[None, :, 1]) + d[:, None, 2] * c[None, :, 2]


def hit_table(verts, faces, origin, dirs, chunk=256):
    """per (ray, face): (t as float32, inf where there is no hit; the near-edge flag of the module docstring)"""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    o = np.asarray(origin, np.float32).astype(np.float64)
    d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    R, F = len(d), len(faces)
    t32 = np.full((R, F), np.inf, np.float32)
    near = np.zeros((R, F), bool)
    for f0 in range(0, F, chunk):
        fc = faces[f0:f0 + chunk]
        a, b, c = verts[fc[:, 0]] - o, verts[fc[:, 1]] - o, verts[fc[:, 2]] - o
        cbc = _cross_ordered(b, fc[:, 1], c, fc[:, 2])
        cca = _cross_ordered(c, fc[:, 2], a, fc[:, 0])
        cab = _cross_ordered(a, fc[:, 0], b, fc[:, 1])
        n = _cross(b - a, c - a)
        na = (n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]
        with np.errstate(all="ignore"):
            e0, e1, e2 = _dot(d, cbc), _dot(d, cca), _dot(d, cab)
            pos = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
            neg = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
            den = _dot(d, n)
            t = na[None] / den
            front = ((den > 0) | (den < 0)) & (t > 0)
            hit = (pos ^ neg) & front
            s = (e0 + e1) + e2
            u = np.stack([e0 / s, e1 / s, e2 / s])
            near[:, f0:f0 + chunk] = front & ~((u.min(0) < -BARY_MARGIN) | (u.min(0) > BARY_MARGIN))   # NaN counts as near
        t32[:, f0:f0 + chunk] = np.where(hit, t.astype(np.float32), np.float32(np.inf))
    return t32, near


def first_hit(verts, faces, k_inv, c2w, mask, return_close=False):
    """face_id (H,W) int32: the face with the smallest float32 t (ties: the lowest index) for every pixel of ``mask``, else -1"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    face_id = np.full((H, W), -1, np.int32)
    close = np.zeros((H, W), bool)
    faces = np.asarray(faces).reshape(-1, 3)
    if mask.any() and len(faces):
        o, d = rays(k_inv, c2w, H, W)
        t32, near = hit_table(verts, faces, o, d[mask])
        best = t32.argmin(1)                                  # the first minimum: the lowest face index
        tb = t32[np.arange(len(best)), best]
        face_id[mask] = np.where(np.isfinite(tb), best, -1)
        if return_close:
            cl = near.any(1)
            if t32.shape[1] > 1:
                two = np.partition(t32.astype(np.float64), 1, axis=1)[:, :2]
                with np.errstate(all="ignore"):
                    cl |= np.isfinite(two[:, 1]) & ((two[:, 1] - two[:, 0]) < T_MARGIN * two[:, 1])
            close[mask] = cl
    return (face_id, close) if return_close else face_id


# ------------------------------------------------------------------ stage 4: components
def merged_vertex_ids(verts):
    """vertices with exactly equal coordinates are one vertex"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    if len(verts) == 0:
        return np.zeros(0, np.int64)
    return np.unique(verts + 0.0, axis=0, return_inverse=True)[1].reshape(-1)     # + 0.0: -0.0 and 0.0 are equal


def face_adjacency(verts, faces):
    """(M,2) face pairs: undirected edges (of merged vertices) that exactly two faces have; degenerate faces have no edges"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = merged_vertex_ids(verts)[faces]
    good = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 2] != ids[:, 0])
    fidx = np.repeat(np.arange(len(faces)), 3)
    e = np.sort(np.stack([ids, np.roll(ids, -1, 1)], -1).reshape(-1, 2), 1)
    keep = np.repeat(good, 3)
    e, fidx = e[keep], fidx[keep]
    if len(e) == 0:
        return np.zeros((0, 2), np.int64)
    uniq, inv, cnt = np.unique(e, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])[cnt == 2]
    return np.stack([fidx[order[starts]], fidx[order[starts + 1]]], 1)


def components(verts, faces):
    """labels (F,) int32: the lowest face index of the face's component, -1 without adjacency"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    F = len(np.asarray(faces).reshape(-1, 3))
    adj = face_adjacency(verts, faces)
    labels = np.full(F, -1, np.int32)
    if len(adj) == 0:
        return labels
    g = coo_matrix((np.ones(len(adj)), (adj[:, 0], adj[:, 1])), shape=(F, F))
    _, comp = connected_components(g, directed=False)
    lowest = np.full(comp.max() + 1, F, np.int64)
    np.minimum.at(lowest, comp, np.arange(F))
    has = np.zeros(F, bool)
    has[adj.reshape(-1)] = True
    labels[has] = lowest[comp[has]]
    return labels


def keep_by_components(verts, faces, labels, min_faces=500, largest_only=False):
    """(vertices, faces) of the components with >= min_faces faces; unreferenced vertices dropped, order preserved"""
    verts, faces = np.asarray(verts), np.asarray(faces).reshape(-1, 3)
    F = len(faces)
    size = np.bincount(labels[labels >= 0], minlength=max(F, 1))
    keep = (labels >= 0) & (size[labels.clip(0)] >= min_faces)
    if largest_only and keep.any():
        cand = np.where(size >= max(min_faces, 1), size, 0)
        keep &= labels == int(cand.argmax())                  # argmax: the first maximum, the lowest label
    f = faces[keep]
    used = np.zeros(len(verts), bool)
    used[f.reshape(-1)] = True
    index = np.cumsum(used) - 1
    return verts[used], index[f].astype(np.int32)


# ------------------------------------------------------------------ the whole pipeline
def clean_mesh(verts, faces, cams, masks, minimal_vis=1, mask_dilated_size=11, min_faces=500, largest_only=False):
    """cams: (K 3x3, E 4x4) float32 pairs as in a *_cam.txt; masks: (H,W) uint8 images.  Returns a dict of every stage."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    dil = [dilated_mask(m, mask_dilated_size) for m in masks]
    Ps = [projection(K, E) for K, E in cams]
    votes = vertex_votes(verts, Ps, dil)
    v2, f2, _ = keep_by_votes(verts, faces, votes, minimal_vis)
    hit = np.zeros(len(f2), bool)
    ids, close = [], []
    for (K, E), m in zip(cams, dil):
        Kn, c2w = camera(K, E)
        fid, cl = first_hit(v2, f2, k_inverse(Kn), c2w, m, return_close=True)
        ids.append(fid)
        close.append(cl)
        hit[fid[fid >= 0]] = True
    f3 = f2[hit]
    labels = components(v2, f3)
    v4, f4 = keep_by_components(v2, f3, labels, min_faces, largest_only)
    return dict(dilated=dil, votes=votes, verts2=v2, faces2=f2, face_ids=ids, close=close, faces3=f3, labels=labels,
                verts=v4, faces=f4)
