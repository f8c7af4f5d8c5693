"""Mesh fly-through on the GPU: the reference's render_trajectory_dtu.py and render_trajectory_open3d.py, which turn a
reconstructed mesh into the 240-frame camera sweep of the reference's README, without Open3D, OpenGL or a display.  The camera
path is numpy float64; every pixel is HIP (csrc/mesh_clean.hip's first hit, then csrc/raster.hip through
``ops.raster_vertex_normals``, ``ops.raster_frames`` and ``ops.raster_downsample``); include/ufr.h states every rule.

    python -m uforecon_amd.render_trajectory --mesh_dir OUT/mesh/final --root_dir DTU_TEST --out_dir OUT/rendering
        [--scans ... --views 23 24 23 --num_views 240 --img_wh 800 640 --original_img_wh 1600 1200 --offset_dist 25
         --supersample 2 --flat --color vertex|uniform|texture --ambient A --format jpg|png --quality 90 --dump_poses DIR]

reads ``<mesh_dir>/scan<N>.ply`` and ``<root_dir>/cameras/<view>_cam.txt`` and writes ``<out_dir>/scan<N>/render_<i>.jpg``.
``--color texture`` reads ``<mesh_dir>/scan<N>.obj`` with its material and PNG instead, as ``texture_mesh`` writes them, and
takes every pixel's colour from the atlas (bilinear, no mipmaps: ``--supersample`` is the antialiasing).

1. key poses as ``DtuFitSparse.load_scene`` builds ``all_render_w2cs_original``: ``c2w = inv(E)`` in float64, moved by
   ``offset_dist`` along its own x axis; the path is ``interpolate_trajectory`` of the reference (scipy's ``Slerp`` for the
   rotation, linear positions), restated here so that scipy is not needed at run time;
2. intrinsics: the first view's K with row 0 scaled by ``img_w / original_w`` and row 1 by ``img_h / original_h``;
3. per frame the first hit of every pixel's ray, then shading: a headlight, ``I = ambient + (1 - ambient) |N . d|``, two-sided
   (marching-cubes meshes come with either winding), smooth (area-weighted vertex normals) or ``--flat``; white like the
   reference's painted mesh, or the PLY's vertex colours (``--color vertex``);
4. ``--supersample s`` renders at s x the size and box-filters down.

Differences from the reference, all deliberate: the reference renders through an Open3D ``Visualizer`` window with a light set by
``render.json`` (not in its tree); the shading here is this module's own rule, not a copy of that window's.  The reference holds
the key poses in float32; here they stay float64 until the ray generator narrows them.  ``--dump_poses`` writes the Open3D
pinhole-camera JSON of every frame (the fields the reference fills), so that the path can be replayed where Open3D exists.

Point clouds (the chain's ``pcd/scan<N>.ply`` of depth_fusion and tsdf, dtu_eval's error clouds) go through the same path, sizes
and files, which the reference has no script for:

    python -m uforecon_amd.render_trajectory --pcd_dir OUT/pcd --root_dir DTU_TEST --out_dir OUT/rendering
        [--ply FILE ... --point_radius 1 --edl 200 --color vertex|uniform  and the flags above but --flat / --ambient]

``render_points``: a z-buffered splat (one thread per point, a 64-bit atomic minimum of depth bits and index per covered pixel)
and a resolve with eye-dome lighting (csrc/splat.hip through ``ops.splat_frames``); tests/points_ref.py is the numpy statement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from .clean_mesh import ray_camera, read_cam_file
from .dtu_eval import DTU_SCANS, read_ply

VIEWS = [23, 24, 23]
NUM_VIEWS = 240
IMG_WH = [800, 640]
ORIGINAL_IMG_WH = [1600, 1200]
OFFSET_DIST = 25.0
# eye-dome lighting strength of render_points.  Derived, not tuned on a real scan: a depth step of 1 % of the depth at one of
# the four neighbours contributes log2(1.01) / 4 = 0.00359 to the exponent, and ln 2 / 0.00359 = 193 halves the brightness there.
DEFAULT_EDL = 200.0


# ------------------------------------------------------------------ the camera path
def _quat_from_matrix(R):
    """unit quaternion (x, y, z, w) of a rotation matrix, from its largest of trace / diagonal entries (as scipy's from_matrix)"""
    d = [R[0, 0], R[1, 1], R[2, 2], R[0, 0] + R[1, 1] + R[2, 2]]
    c = int(np.argmax(d))
    q = np.empty(4)
    if c == 3:
        q[0], q[1], q[2], q[3] = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1 + d[3]
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1 - d[3] + 2 * R[i, i]
        q[j] = R[j, i] + R[i, j]
        q[k] = R[k, i] + R[i, k]
        q[3] = R[k, j] - R[j, k]
    return q / np.sqrt(q @ q)


def _quat_mul(p, q):
    """p q, (x, y, z, w)"""
    return np.array([p[3] * q[0] + q[3] * p[0] + (p[1] * q[2] - p[2] * q[1]),
                     p[3] * q[1] + q[3] * p[1] + (p[2] * q[0] - p[0] * q[2]),
                     p[3] * q[2] + q[3] * p[2] + (p[0] * q[1] - p[1] * q[0]),
                     p[3] * q[3] - (p[0] * q[0] + p[1] * q[1] + p[2] * q[2])])


def _rotvec_from_quat(q):
    """log: the rotation vector of the shorter way round (w >= 0), by series below 1e-3 rad"""
    if q[3] < 0:
        q = -q
    s = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    angle = 2 * np.arctan2(s, q[3])
    if angle <= 1e-3:
        a2 = angle * angle
        scale = 2 + a2 / 12 + 7 * a2 * a2 / 2880
    else:
        scale = angle / np.sin(angle / 2)
    return scale * q[:3]


def _quat_from_rotvec(r):
    """exp"""
    angle = np.sqrt(r @ r)
    if angle <= 1e-3:
        a2 = angle * angle
        scale = 0.5 - a2 / 48 + a2 * a2 / 3840
    else:
        scale = np.sin(angle / 2) / angle
    return np.array([scale * r[0], scale * r[1], scale * r[2], np.cos(angle / 2)])


def _matrix_from_quat(q):
    x, y, z, w = q
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                     [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                     [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]])


def interpolate_trajectory(w2cs, num_views: int = NUM_VIEWS):
    """The reference's ``interpolate_trajectory`` (render_trajectory_dtu.py:57-77) in numpy float64: ``w2cs`` (K,4,4), K >= 2 key
    cameras at times 0..K-1; frame i is at t = i / num_views * (K - 1) (the last key is never reached).  On the segment
    k = floor(t), alpha = t - k the rotation is ``R_k exp(alpha log(R_k^-1 R_k+1))`` (scipy's ``Slerp``: the shorter way
    round), the position linear between the two keys.  Returns (num_views,4,4) float64 camera-to-world matrices.  Equal
    neighbouring keys and a first key equal to the last are fine."""
    w2cs = np.asarray(w2cs, np.float64)
    if w2cs.ndim != 3 or w2cs.shape[1:] != (4, 4) or len(w2cs) < 2:
        raise ValueError(f"interpolate_trajectory: w2cs {w2cs.shape}: expected (K, 4, 4) with K >= 2")
    num_views = int(num_views)
    if num_views < 1:
        raise ValueError(f"interpolate_trajectory: num_views {num_views} (must be >= 1)")
    c2ws = np.linalg.inv(w2cs)
    K = len(c2ws)
    quats = [_quat_from_matrix(c[:3, :3]) for c in c2ws]
    conj = np.array([-1.0, -1.0, -1.0, 1.0])
    rotvecs = [_rotvec_from_quat(_quat_mul(quats[k] * conj, quats[k + 1])) for k in range(K - 1)]
    out = np.empty((num_views, 4, 4))
    for i in range(num_views):
        t = float(i) / num_views * (K - 1)
        k = min(int(np.floor(t)), K - 2)
        alpha = t - k
        c2w = np.eye(4)
        c2w[:3, :3] = _matrix_from_quat(_quat_mul(quats[k], _quat_from_rotvec(alpha * rotvecs[k])))
        c2w[:3, 3] = c2ws[k, :3, 3] + (c2ws[k + 1, :3, 3] - c2ws[k, :3, 3]) * alpha
        out[i] = c2w
    return out


def key_poses(root_dir, views=VIEWS, offset_dist=OFFSET_DIST):
    """(K 3x3 float32 of the first view, w2cs (len(views),4,4) float64): the key cameras as ``DtuFitSparse.load_scene`` builds
    ``all_render_w2cs_original`` -- c2w = inv(E) in float64, moved by ``offset_dist`` along its own x axis."""
    w2cs, K0 = [], None
    for v in views:
        K, E = read_cam_file(os.path.join(root_dir, "cameras/{:0>8}_cam.txt".format(v)))
        if K0 is None:
            K0 = K
        c2w = np.linalg.inv(E.astype(np.float64))
        c2w[:3, 3] += c2w[:3, 0] * offset_dist
        w2cs.append(np.linalg.inv(c2w))
    return K0, np.stack(w2cs)


def scaled_intrinsics(K, img_wh=IMG_WH, original_img_wh=ORIGINAL_IMG_WH):
    """K (float64) with row 0 multiplied by img_w / original_w and row 1 by img_h / original_h"""
    K = np.asarray(K, np.float32).astype(np.float64)[:3, :3].copy()
    K[0] *= img_wh[0] / original_img_wh[0]
    K[1] *= img_wh[1] / original_img_wh[1]
    return K


def pinhole_json(K, c2w, H, W):
    """The Open3D PinholeCameraParameters dict of one frame, the fields the reference fills: ``extrinsic`` = the w2c flattened
    column-major, ``intrinsic.intrinsic_matrix`` column-major, ``width``, ``height``."""
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    return {"class_name": "PinholeCameraParameters", "extrinsic": w2c.T.reshape(-1).tolist(),
            "intrinsic": {"height": int(H), "intrinsic_matrix": np.asarray(K, np.float64)[:3, :3].T.reshape(-1).tolist(),
                          "width": int(W)},
            "version_major": 1, "version_minor": 0}


def load_pinhole_json(path):
    """(K 3x3, c2w 4x4, H, W) of a file ``pinhole_json`` wrote (the reference's ``load``)"""
    with open(path) as f:
        j = json.load(f)
    w2c = np.array(j["extrinsic"], np.float64).reshape(4, 4).T
    K = np.array(j["intrinsic"]["intrinsic_matrix"], np.float64).reshape(3, 3).T
    return K, np.linalg.inv(w2c), int(j["intrinsic"]["height"]), int(j["intrinsic"]["width"])


# ------------------------------------------------------------------ rendering
def supersampled_intrinsics(K, s):
    """K' = [[s, 0, (s-1)/2], [0, s, (s-1)/2], [0, 0, 1]] K: pixel centres are integers, so pixel x of the small image covers
    the big image's s x - 1/2 + (1/2 .. s - 1/2), whose centres are s x + 0 .. s - 1"""
    S = np.array([[s, 0, (s - 1) / 2], [0, s, (s - 1) / 2], [0, 0, 1]], np.float64)
    return S @ np.asarray(K, np.float64)[:3, :3]


def _frames_per_chunk(n, H, W, s, extra_bytes_per_pixel, device):
    import torch

    per_frame = (s * H) * (s * W) * 3 + H * W * (3 + extra_bytes_per_pixel)
    free = torch.cuda.mem_get_info(device)[0] if torch.cuda.is_available() else 1 << 30
    return max(1, min(n, int(free // 4 // per_frame)))   # a quarter of what is free: the allocator and the workspace need room


def render_mesh(verts, faces, K, c2ws, H, W, colors=None, smooth=True, ambient=0.25, base_color=(1, 1, 1),
                background=(255, 255, 255), supersample=1, return_depth=False, return_normals=False, return_face_ids=False,
                device="cuda", texture=None, corner_xy=None):
    """Shaded views of a mesh: uint8 (n,H,W,3) images as a numpy array.  ``verts`` (V,3) any float dtype, ``faces`` (F,3)
    integers, ``K`` 3x3 intrinsics (normalised and inverted as ``clean_mesh.ray_camera`` does), ``c2ws`` (n,4,4) or (4,4)
    camera-to-world matrices, ``colors`` (V,3) uint8 vertex colours or None (``base_color``, 0..1).  ``texture`` (Ht,Wt,3)
    uint8 with ``corner_xy`` (F,3,2) texel coordinates of every face's corners, as ``texture_mesh.texture_mesh`` returns them:
    the colour comes from the texture (``texture_ops.raster_frames_textured``; ``colors`` must then be None).  ``smooth``: area-weighted
    vertex normals, else the face normal.  ``supersample`` s in 1..4 renders at s x the size and box-filters down.  With
    ``return_depth`` / ``return_normals`` / ``return_face_ids`` a tuple: the images, then float32 (n,H,W) z-depth (0: no hit),
    float32 (n,H,W,3) camera-space normals facing the camera, int32 (n,H,W) face ids (-1: no hit), in that order -- at
    ``supersample=1`` only.  The frames are rendered in chunks sized from free device memory; one host synchronisation per
    chunk, none per frame."""
    import torch

    from . import ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    c2ws = np.asarray(c2ws, np.float64)
    if c2ws.ndim == 2:
        c2ws = c2ws[None]
    s, H, W = int(supersample), int(H), int(W)
    extras = [k for k, on in (("depth", return_depth), ("normal", return_normals), ("face_id", return_face_ids)) if on]
    if not 1 <= s <= 4:
        raise UfrError(f"render_mesh: supersample {supersample} (must be 1 .. 4)")
    if extras and s != 1:
        raise UfrError("render_mesh: depth, normal and face-id maps are only available at supersample=1")
    if c2ws.ndim != 3 or c2ws.shape[1:] != (4, 4) or len(c2ws) < 1:
        raise UfrError(f"render_mesh: c2ws {c2ws.shape}: expected (n, 4, 4) with n >= 1")
    if H < 1 or W < 1:
        raise UfrError(f"render_mesh: image {H}x{W} (H and W must be >= 1)")
    V, F = len(verts), len(faces)
    if F and (V == 0 or faces.min() < 0 or faces.max() >= V):
        raise UfrError(f"render_mesh: face indices span {faces.min()}..{faces.max()}, the mesh has {V} vertices")
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != (V, 3) or colors.dtype != np.uint8:
            raise UfrError(f"render_mesh: colors {colors.shape} {colors.dtype}: expected ({V}, 3) uint8")
    if (texture is None) != (corner_xy is None) or (texture is not None and colors is not None):
        raise UfrError("render_mesh: texture and corner_xy come together, and without colors")
    if texture is not None:
        texture, corner_xy = np.asarray(texture), np.asarray(corner_xy, np.float64)
        if texture.ndim != 3 or texture.shape[2] != 3 or texture.dtype != np.uint8 or corner_xy.shape != (F, 3, 2):
            raise UfrError(f"render_mesh: texture {texture.shape} {texture.dtype}, corner_xy {corner_xy.shape}: expected (Ht, Wt, 3) "
                           f"uint8 and ({F}, 3, 2)")
    dev = torch.device(device)
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)
    tc = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
    tt = txy = None
    if texture is not None:
        from . import texture_ops

        tt = torch.from_numpy(np.ascontiguousarray(texture)).to(dev)
        txy = torch.from_numpy(np.ascontiguousarray(corner_xy)).to(dev)
    tn = ops.raster_vertex_normals(tv, tf) if smooth and F else None
    k_inv = ray_camera(supersampled_intrinsics(K, s).astype(np.float32), np.eye(4, dtype=np.float32))[0]
    n = len(c2ws)
    chunk = _frames_per_chunk(n, H, W, s, 4 * return_depth + 12 * return_normals + 4 * return_face_ids, dev)
    out = {k: [] for k in ["image"] + extras}
    for i in range(0, n, chunk):
        want = dict(background=background, ambient=ambient, return_depth=return_depth, return_face_ids=return_face_ids,
                    return_normals=return_normals, check_indices=False)
        if tt is not None:
            r = texture_ops.raster_frames_textured(tv, tf, k_inv, c2ws[i:i + chunk], s * H, s * W, txy, tt, normals=tn, **want)
        else:
            r = ops.raster_frames(tv, tf, k_inv, c2ws[i:i + chunk], s * H, s * W, normals=tn, colors=tc, base_color=base_color,
                                  **want)
        if s > 1:
            r["image"] = ops.raster_downsample(r["image"], s)
        for k in out:
            out[k].append(r[k].cpu().numpy())
    res = [np.concatenate(out[k]) for k in ["image"] + extras]
    return res[0] if not extras else tuple(res)


def render_points(points, K, c2ws, H, W, colors=None, radius=1, edl_strength=DEFAULT_EDL, edl_radius=None, base_color=(1, 1, 1),
                  background=(255, 255, 255), supersample=1, return_depth=False, return_point_ids=False, device="cuda"):
    """Splat views of a point cloud, the sibling of ``render_mesh``: uint8 (n,H,W,3) images as a numpy array.  ``points`` (N,3)
    any float dtype, ``K`` 3x3 intrinsics (divided by ``K[2,2]`` as ``clean_mesh.ray_camera`` does), ``c2ws`` (n,4,4) or (4,4)
    camera-to-world matrices (inverted here in float64), ``colors`` (N,3) uint8 or None (``base_color``, 0..1).  Every point
    covers the pixels within ``radius`` (0..4) of its projection, the nearest point wins a pixel, and eye-dome lighting darkens
    a pixel by how far it lies behind its four neighbours at distance ``edl_radius`` in log depth (``edl_strength=0``: none).
    ``supersample`` s in 1..4 renders at s x the size with radius ``s * radius + (s - 1)`` (capped at 4) and ``edl_radius``
    defaulting to s, so that a dot keeps its screen size, and box-filters down.  With ``return_depth`` / ``return_point_ids``
    a tuple: the images, then float32 (n,H,W) z-depth (0: empty), int32 (n,H,W) point ids (-1: empty) -- at ``supersample=1``
    only.  An empty cloud gives background frames.  Chunked from free device memory as ``render_mesh`` is."""
    import torch

    from . import ops
    from ._lib import UfrError

    points = np.asarray(points, np.float64).reshape(-1, 3)
    c2ws = np.asarray(c2ws, np.float64)
    if c2ws.ndim == 2:
        c2ws = c2ws[None]
    s, H, W, radius = int(supersample), int(H), int(W), int(radius)
    extras = [k for k, on in (("depth", return_depth), ("point_id", return_point_ids)) if on]
    if not 1 <= s <= 4:
        raise UfrError(f"render_points: supersample {supersample} (must be 1 .. 4)")
    if extras and s != 1:
        raise UfrError("render_points: depth and point-id maps are only available at supersample=1")
    if c2ws.ndim != 3 or c2ws.shape[1:] != (4, 4) or len(c2ws) < 1:
        raise UfrError(f"render_points: c2ws {c2ws.shape}: expected (n, 4, 4) with n >= 1")
    if H < 1 or W < 1:
        raise UfrError(f"render_points: image {H}x{W} (H and W must be >= 1)")
    if not 0 <= radius <= 4:
        raise UfrError(f"render_points: radius {radius} (must be 0 .. 4)")
    edl_radius = s if edl_radius is None else int(edl_radius)
    if edl_radius < 1 or not (float(edl_strength) >= 0.0 and np.isfinite(float(edl_strength))):
        raise UfrError(f"render_points: edl_strength {edl_strength}, edl_radius {edl_radius} (must be finite and >= 0, and >= 1)")
    N, n = len(points), len(c2ws)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != (N, 3) or colors.dtype != np.uint8:
            raise UfrError(f"render_points: colors {colors.shape} {colors.dtype}: expected ({N}, 3) uint8")
    if N == 0:
        bg = np.asarray(background).reshape(-1)
        if bg.shape != (3,) or not ((bg >= 0) & (bg <= 255) & (bg == np.rint(bg))).all():
            raise UfrError(f"render_points: background {background!r} (three integers in 0 .. 255)")
        res = [np.broadcast_to(bg.astype(np.uint8), (n, H, W, 3)).copy()]
        res += [np.zeros((n, H, W), np.float32) if k == "depth" else np.full((n, H, W), -1, np.int32) for k in extras]
        return res[0] if not extras else tuple(res)
    Ks = supersampled_intrinsics(K, s)
    if not np.isfinite(Ks).all() or Ks[2, 2] == 0:
        raise UfrError("render_points: K is not finite or K[2,2] is 0")
    Ks = Ks / Ks[2, 2]
    try:
        w2cs = np.linalg.inv(c2ws)
    except np.linalg.LinAlgError:
        raise UfrError("render_points: a camera-to-world matrix is singular") from None
    if not (np.isfinite(c2ws).all() and np.isfinite(w2cs).all()):
        raise UfrError("render_points: a camera-to-world matrix is singular or not finite")
    dev = torch.device(device)
    tp = torch.from_numpy(np.ascontiguousarray(points)).to(dev)
    tc = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
    chunk = _frames_per_chunk(n, H, W, s, 4 * return_depth + 4 * return_point_ids, dev)
    out = {k: [] for k in ["image"] + extras}
    for i in range(0, n, chunk):
        r = ops.splat_frames(tp, Ks, w2cs[i:i + chunk], s * H, s * W, colors=tc, radius=min(4, s * radius + (s - 1)),
                             base_color=base_color, background=background, edl_strength=edl_strength, edl_radius=edl_radius,
                             return_depth=return_depth, return_point_ids=return_point_ids)
        if s > 1:
            r["image"] = ops.raster_downsample(r["image"], s)
        for k in out:
            out[k].append(r[k].cpu().numpy())
    res = [np.concatenate(out[k]) for k in ["image"] + extras]
    return res[0] if not extras else tuple(res)


# ------------------------------------------------------------------ the command line
def make_parser():
    """The reference's constants (render_trajectory_dtu.py:93-107, 134) as defaults."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh_dir", type=str, default="./outputs/mesh/final", help="directory of scan<N>.ply")
    parser.add_argument("--root_dir", type=str, default="./dtu_test", help="dataset (cameras/<view>_cam.txt)")
    parser.add_argument("--out_dir", type=str, default="./rendering", help="frames go to <out_dir>/scan<N>/")
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    parser.add_argument("--views", type=int, nargs="+", default=VIEWS, help="key views of the path (the reference: 23 24 23)")
    parser.add_argument("--num_views", type=int, default=NUM_VIEWS, help="frames of the path")
    parser.add_argument("--img_wh", type=int, nargs=2, default=IMG_WH, help="rendered width and height")
    parser.add_argument("--original_img_wh", type=int, nargs=2, default=ORIGINAL_IMG_WH, help="size the camera files' K refers to")
    parser.add_argument("--offset_dist", type=float, default=OFFSET_DIST, help="sideways shift of the key cameras (mm)")
    parser.add_argument("--supersample", type=int, default=1, choices=[1, 2, 3, 4])
    parser.add_argument("--flat", action="store_true", help="face normals instead of smooth vertex normals")
    parser.add_argument("--color", choices=["vertex", "uniform", "texture"], default="uniform",
                        help="vertex: the PLY's red/green/blue; texture: <mesh_dir>/scan<N>.obj with its PNG (texture_mesh)")
    parser.add_argument("--ambient", type=float, default=0.25)
    parser.add_argument("--format", choices=["jpg", "png"], default="jpg")
    parser.add_argument("--quality", type=int, default=90, help="JPEG quality")
    parser.add_argument("--dump_poses", type=str, default=None, help="directory for Open3D pinhole-camera JSON (tmp<i>.json)")
    parser.add_argument("--pcd_dir", type=str, default=None, help="render the point clouds <pcd_dir>/scan<N>.ply instead of meshes")
    parser.add_argument("--ply", type=str, nargs="+", default=None,
                        help="render these point-cloud files instead of scan<N>.ply, each to <out_dir>/<file stem>/")
    parser.add_argument("--point_radius", type=int, default=1, choices=[0, 1, 2, 3, 4], help="pixels round a point's projection")
    parser.add_argument("--edl", type=float, default=DEFAULT_EDL,
                        help="eye-dome lighting strength of a point cloud (0: none); the default is derived -- a 1 %% depth step "
                             "at one neighbour halves the brightness -- not tuned on a real scan")
    return parser


def _scan_cameras(root_dir, views, num_views, img_wh, original_img_wh, offset_dist, dump_poses):
    """(K float64 3x3, c2ws (num_views,4,4), H, W) of a path through ``views``; writes the pose files when asked"""
    if len(views) < 2:
        raise ValueError(f"render_scan: views {views}: at least two key views are needed")
    K0, w2cs = key_poses(root_dir, views, offset_dist)
    c2ws = interpolate_trajectory(w2cs, num_views)
    K = scaled_intrinsics(K0, img_wh, original_img_wh)
    W, H = int(img_wh[0]), int(img_wh[1])
    if dump_poses:
        os.makedirs(dump_poses, exist_ok=True)
        for i, c2w in enumerate(c2ws):
            with open(os.path.join(dump_poses, "tmp%d.json" % i), "w") as f:
                json.dump(pinhole_json(K, c2w, H, W), f, indent=4)
    return K, c2ws, H, W


def _write_frames(images, out_dir, fmt, quality):
    from PIL import Image

    os.makedirs(out_dir, exist_ok=True)
    for i, img in enumerate(images):
        path = os.path.join(out_dir, "render_%d.%s" % (i, fmt))
        if fmt == "jpg":
            Image.fromarray(img).save(path, quality=quality)
        else:
            Image.fromarray(img).save(path)


def render_scan(mesh_path, root_dir, out_dir, views=VIEWS, num_views=NUM_VIEWS, img_wh=IMG_WH, original_img_wh=ORIGINAL_IMG_WH,
                offset_dist=OFFSET_DIST, supersample=1, flat=False, color="uniform", ambient=0.25, fmt="jpg", quality=90,
                dump_poses=None):
    """One scan: the frames ``<out_dir>/render_<i>.<fmt>`` of ``mesh_path`` along the path through ``views``.  Returns the
    (num_views,4,4) camera-to-world matrices.  ``color="texture"``: ``mesh_path`` is an OBJ of ``texture_mesh.write_obj``."""
    texture = corner_xy = None
    if color == "texture":
        from .texture_mesh import read_obj

        verts, faces, corner_xy, texture = read_obj(mesh_path)
        colors = None
    else:
        verts, faces, colors = read_ply(mesh_path, with_colors=True)
    if faces is None:
        faces = np.zeros((0, 3), np.int32)
    K, c2ws, H, W = _scan_cameras(root_dir, views, num_views, img_wh, original_img_wh, offset_dist, dump_poses)
    images = render_mesh(verts, faces, K, c2ws, H, W, colors=colors if color == "vertex" else None, smooth=not flat,
                         ambient=ambient, supersample=supersample, texture=texture, corner_xy=corner_xy)
    _write_frames(images, out_dir, fmt, quality)
    return c2ws


def render_cloud(ply_path, root_dir, out_dir, views=VIEWS, num_views=NUM_VIEWS, img_wh=IMG_WH, original_img_wh=ORIGINAL_IMG_WH,
                 offset_dist=OFFSET_DIST, supersample=1, color="uniform", point_radius=1, edl=DEFAULT_EDL, fmt="jpg", quality=90,
                 dump_poses=None):
    """``render_scan`` for a point cloud: the vertices of ``ply_path`` (its faces, if any, are ignored) splatted along the same
    path into the same files.  ``color="uniform"`` paints the cloud white and leaves the shading to eye-dome lighting alone
    (a cloud from ``tsdf`` without ``--integrate_color`` carries black vertices); ``"vertex"`` uses the PLY's colours."""
    points, _, colors = read_ply(ply_path, with_colors=True)
    K, c2ws, H, W = _scan_cameras(root_dir, views, num_views, img_wh, original_img_wh, offset_dist, dump_poses)
    images = render_points(points, K, c2ws, H, W, colors=colors if color == "vertex" else None, radius=point_radius,
                           edl_strength=edl, supersample=supersample)
    _write_frames(images, out_dir, fmt, quality)
    return c2ws


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.pcd_dir is not None or args.ply:
        if args.ply:
            jobs = [(os.path.splitext(os.path.basename(p))[0], p) for p in args.ply]
        else:
            jobs = [("scan%d" % scan, os.path.join(args.pcd_dir, "scan%d.ply" % scan)) for scan in args.scans]
        for name, path in jobs:
            if not os.path.exists(path):
                print("%s: no point cloud at %s" % (name, path))
                continue
            print("rendering %s (points)" % name)
            render_cloud(path, args.root_dir, os.path.join(args.out_dir, name), args.views, args.num_views, args.img_wh,
                         args.original_img_wh, args.offset_dist, args.supersample, args.color, args.point_radius, args.edl,
                         args.format, args.quality, args.dump_poses)
        return
    for scan in args.scans:
        mesh = os.path.join(args.mesh_dir, "scan%d.%s" % (scan, "obj" if args.color == "texture" else "ply"))
        if not os.path.exists(mesh):
            print("scan%d: no mesh at %s" % (scan, mesh))
            continue
        print("rendering scan%d" % scan)
        render_scan(mesh, args.root_dir, os.path.join(args.out_dir, "scan%d" % scan), args.views, args.num_views, args.img_wh,
                    args.original_img_wh, args.offset_dist, args.supersample, args.flat, args.color, args.ambient, args.format,
                    args.quality, args.dump_poses)      # the cameras are the dataset's, not the scan's: one set of poses


if __name__ == "__main__":
    sys.exit(main())
