"""numpy float64 restatement of mesh rendering (include/ufr.h, "mesh rendering"; csrc/raster.hip): vertex normals, the shading
of first-hit pixels and the box downsample, with the kernels' expressions and summation orders.  The ray generator, the first
hit and the ordered edge products are clean_mesh_ref.py's, imported as they are.  Slow and plain on purpose.

A pixel is *close* when
  * clean_mesh_ref marks its first hit close (a ray within 1e-6 of an edge or vertex, or two hits within 1e-6 relative in t), or
  * the interpolated vertex normal is shorter than 1e-9 (the smooth / flat decision could fall either way), or
  * some channel's 255 * colour * I lies within 1e-6 of a half-integer (the rounding could fall either way).
"""
import numpy as np

from clean_mesh_ref import BARY_MARGIN, T_MARGIN, _cross, _cross_ordered, first_hit, rays  # noqa: F401

NORMAL_MARGIN = 1e-9
HALF_MARGIN = 1e-6


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def vertex_normals(verts, faces):
    """(V,3) float64: per vertex the sum, in ascending corner-slot order, of (b - a) x (c - a) over the faces that use it,
    divided by its length; zero for an unused vertex or a zero sum; a face with an index outside 0..V-1 contributes nothing"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    ok = ((faces >= 0) & (faces < V)).all(1)
    f = faces[ok]
    a = verts[f[:, 0]]
    n = _cross(verts[f[:, 1]] - a, verts[f[:, 2]] - a)
    s = np.zeros((V, 3))
    for k in range(3):                                       # np.add.at is unbuffered: it adds in the order of the index array,
        np.add.at(s[:, k], f.reshape(-1), np.repeat(n[:, k], 3))   # which is ascending slot order 3f + e
    with np.errstate(all="ignore"):
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        good = np.isfinite(ln) & (ln > 0)
        return np.where(good[:, None], s / ln[:, None], 0.0)


def camera_unit_rays(k_inv, H, W):
    """v (H,W,3) float32: the camera-space unit rays, the expressions of clean_mesh_ref.rays"""
    ki = np.asarray(k_inv, np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    one = np.float32(1)
    p = [(ki[i, 0] * xs + ki[i, 1] * ys) + ki[i, 2] * one for i in range(3)]
    n = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
    v = np.stack([c / n for c in p], -1)
    assert v.dtype == np.float32
    return v


def render(verts, faces, k_inv, c2w, H, W, normals=None, colors=None, base_color=(1.0, 1.0, 1.0), ambient=0.25,
           background=(255, 255, 255), hit=None):
    """One frame: dict of image (H,W,3) uint8, depth (H,W) float32, face_id (H,W) int32, normal (H,W,3) float32, close (H,W)
    bool.  ``normals`` (V,3) float64 or None (flat), ``colors`` (V,3) uint8 or None (``base_color``).  ``hit``: the
    ``(face_id, close)`` pair of an earlier call with the same mesh and camera (the brute-force first hit is the slow part)."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cw = np.asarray(c2w, np.float32)
    face_id, close = hit if hit is not None else first_hit(verts, faces, k_inv, c2w, np.ones((H, W), bool), return_close=True)
    image = np.empty((H, W, 3), np.uint8)
    image[:] = np.asarray(background, np.uint8)
    depth = np.zeros((H, W), np.float32)
    normal = np.zeros((H, W, 3), np.float32)
    on = face_id >= 0
    if on.any():
        o, d32 = rays(k_inv, c2w, H, W)
        o = o.astype(np.float64)
        d = d32[on].astype(np.float64)
        vz = camera_unit_rays(k_inv, H, W)[on][:, 2].astype(np.float64)
        fc = faces[face_id[on]]
        a, b, c = verts[fc[:, 0]] - o, verts[fc[:, 1]] - o, verts[fc[:, 2]] - o
        e0 = _dot(d, _cross_ordered(b, fc[:, 1], c, fc[:, 2]))
        e1 = _dot(d, _cross_ordered(c, fc[:, 2], a, fc[:, 0]))
        e2 = _dot(d, _cross_ordered(a, fc[:, 0], b, fc[:, 1]))
        s = (e0 + e1) + e2
        w0, w1, w2 = e0 / s, e1 / s, e2 / s
        n = _cross(b - a, c - a)
        t = _dot(n, a) / _dot(n, d)
        depth[on] = (t * vz).astype(np.float32)
        N = n / np.sqrt(_dot(n, n))[:, None]
        cl = np.zeros(len(d), bool)
        if normals is not None:
            normals = np.asarray(normals, np.float64)
            Ns = (w0[:, None] * normals[fc[:, 0]] + w1[:, None] * normals[fc[:, 1]]) + w2[:, None] * normals[fc[:, 2]]
            ln = np.sqrt(_dot(Ns, Ns))
            with np.errstate(all="ignore"):
                N = np.where((ln > 0)[:, None], Ns / ln[:, None], N)
            cl |= ln < NORMAL_MARGIN
        cd = _dot(N, d)
        I = ambient + (1.0 - ambient) * np.abs(cd)
        if colors is None:
            col = np.broadcast_to(np.asarray(base_color, np.float32).astype(np.float64), (len(d), 3))
        else:
            C = np.asarray(colors, np.uint8).astype(np.float64)
            col = ((w0[:, None] * C[fc[:, 0]] + w1[:, None] * C[fc[:, 1]]) + w2[:, None] * C[fc[:, 2]]) / 255.0
        val = (255.0 * col) * I[:, None]
        image[on] = np.clip(np.rint(val), 0, 255).astype(np.uint8)          # np.rint: half to even
        cl |= (np.abs(np.abs(val - np.floor(val)) - 0.5) < HALF_MARGIN).any(1)
        R = cw[:3, :3].astype(np.float64)
        nc = np.stack([(R[0, j] * N[:, 0] + R[1, j] * N[:, 1]) + R[2, j] * N[:, 2] for j in range(3)], 1)
        normal[on] = np.where((cd > 0)[:, None], -nc, nc).astype(np.float32)
        close = close.copy()
        close[on] |= cl
    return dict(image=image, depth=depth, face_id=face_id, normal=normal, close=close)


def downsample(images, s):
    """(n,sH,sW,3) uint8 -> (n,H,W,3) uint8: block means in integers, round half to even"""
    images = np.asarray(images, np.uint8)
    n, sH, sW, _ = images.shape
    H, W = sH // s, sW // s
    tot = images.reshape(n, H, s, W, s, 3).astype(np.int64).sum((2, 4))
    n2 = s * s
    q, r = tot // n2, tot % n2
    up = (2 * r > n2) | ((2 * r == n2) & (q % 2 == 1))
    return (q + up).astype(np.uint8)
