"""Pictures of a COLMAP camera with lens distortion, resampled to a pinhole camera: the host form of ufr_image_undistort_u8
(csrc/undistort.hip), the zoom that keeps blank pixels out of the result, and the call that picks the kernel or the host form
by device.  `colmap2mvsnet --undistort` is the caller.

The rule is stated in include/ufr.h and followed here operation by operation, in float64 numpy (numpy fuses nothing, so each
product, sum and quotient is rounded on its own, as the kernel rounds them).  It restates COLMAP's public camera models and was
compared with neither COLMAP nor OpenCV: the rule written there is the rule.

A model's parameters reach the three formulas as a family and eight coefficients, a coefficient the model does not have being 0
(adding a zero term changes no finite result):

  polynomial  SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV           k1 k2 p1 p2
  rational    FULL_OPENCV                                                      k1 k2 p1 p2 k3 k4 k5 k6
  fisheye     OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE            k1 k2 k3 k4

FOV and THIN_PRISM_FISHEYE are refused.
"""
from __future__ import annotations

import numpy as np

from .colmap2mvsnet import CAMERA_MODELS, MODEL_IDS, PINHOLE_MODELS, UNDISTORT_FITS  # noqa: F401 (PINHOLE_MODELS: for callers)

FISHEYE_EPS = 1e-8           # below this radius the fisheye scale theta_d / r is taken as 1
ZOOM_MAX = 4.0               # `fit_zoom` looks for its zoom in [1, ZOOM_MAX]
ZOOM_BISECTIONS = 40
GROUP = 8                    # pictures per kernel call
# model -> (family, where its distortion coefficients go among the family's eight)
_FAMILY = {"SIMPLE_PINHOLE": ("polynomial", ()), "PINHOLE": ("polynomial", ()), "SIMPLE_RADIAL": ("polynomial", (0,)),
           "RADIAL": ("polynomial", (0, 1)), "OPENCV": ("polynomial", (0, 1, 2, 3)), "FULL_OPENCV": ("rational", tuple(range(8))),
           "OPENCV_FISHEYE": ("fisheye", (0, 1, 2, 3)), "SIMPLE_RADIAL_FISHEYE": ("fisheye", (0,)), "RADIAL_FISHEYE": ("fisheye", (0, 1))}
SUPPORTED_MODELS = tuple(_FAMILY)


def model_name(model):
    """COLMAP's name of a camera model given by name or id; ValueError for one that is unknown or refused."""
    name = model if isinstance(model, str) else CAMERA_MODELS.get(int(model), (None,))[0]
    if name not in _FAMILY:
        raise ValueError(f"camera model {model} cannot be undistorted (supported: {', '.join(SUPPORTED_MODELS)})")
    return name


def split_params(model, params):
    """((fx, fy, cx, cy), family, k[8]) of a model's COLMAP parameter list."""
    name = model_name(model)
    _, n_params, single = CAMERA_MODELS[MODEL_IDS[name]]
    p = np.asarray(params, np.float64).reshape(-1)
    if p.size != n_params:
        raise ValueError(f"camera model {name} has {n_params} parameters, got {p.size}")
    if not np.isfinite(p).all():
        raise ValueError(f"camera model {name}: a parameter is not finite")
    fxfycxcy = (p[0], p[0], p[1], p[2]) if single else (p[0], p[1], p[2], p[3])
    family, slots = _FAMILY[name]
    k = np.zeros(8)
    k[list(slots)] = p[3 if single else 4:]
    return fxfycxcy, family, k


def distort_host(model, params, x, y):
    """(xd, yd): the model's distortion of the normalised image coordinates ``x``, ``y`` (float64 arrays of one shape)."""
    _, family, k = split_params(model, params)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        xx, yy = x * x, y * y
        r2 = xx + yy
        if family == "fisheye":
            r = np.sqrt(r2)
            t = np.arctan(r)
            t2 = t * t
            t4 = t2 * t2
            t6, t8 = t4 * t2, t4 * t4
            poly = (((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8
            s = np.where(r >= FISHEYE_EPS, (t * poly) / r, 1.0)
            return x * s, y * s
        r4 = r2 * r2
        xy = x * y
        tx = (2.0 * k[2]) * xy + k[3] * (r2 + 2.0 * xx)
        ty = (2.0 * k[3]) * xy + k[2] * (r2 + 2.0 * yy)
        if family == "rational":
            r6 = r4 * r2
            rad = (((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6) / (((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6)
            return x * rad + tx, y * rad + ty
        rad = k[0] * r2 + k[1] * r4
        return (x + x * rad) + tx, (y + y * rad) + ty


def _k_out(k_out):
    k = np.asarray(k_out, np.float64)
    k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]]) if k.shape == (3, 3) else k.reshape(-1)
    if k.size != 4 or not np.isfinite(k).all() or not (k[0] > 0 and k[1] > 0):
        raise ValueError(f"k_out {k_out!r}: expected finite (fx', fy', cx', cy') with positive focal lengths, or that camera's 3x3 matrix")
    return k


def source_map_host(model, params, k_out, Hs, Ws, xs, ys):
    """(u, v, valid) of the output pixels (``xs``, ``ys``) (integer arrays of one shape): where each one's centre lies in the
    (Hs, Ws) source picture, in pixel indices, and whether that is inside it.  ``k_out``: (fx', fy', cx', cy') or the 3x3."""
    (fx, fy, cx, cy), _, _ = split_params(model, params)
    fxo, fyo, cxo, cyo = _k_out(k_out)
    xn = ((np.asarray(xs, np.float64) + 0.5) - cxo) / fxo
    yn = ((np.asarray(ys, np.float64) + 0.5) - cyo) / fyo
    xd, yd = distort_host(model, params, xn, yn)
    with np.errstate(all="ignore"):
        u = (fx * xd + cx) - 0.5
        v = (fy * yd + cy) - 0.5
        valid = (u >= 0.0) & (u <= float(Ws - 1)) & (v >= 0.0) & (v <= float(Hs - 1))         # a NaN fails every comparison
    return u, v, valid


def undistort_host(src, model, params, k_out, H, W, want_valid=True, unrounded=False):
    """ufr_image_undistort_u8 on the host: ``src`` (n,Hs,Ws,C) uint8 -> (dst (n,H,W,C) uint8, valid (H,W) uint8 or None).
    With ``unrounded`` the first item is the float64 value before rint instead (0 where invalid)."""
    src = np.asarray(src)
    H, W = int(H), int(W)
    if src.dtype != np.uint8 or src.ndim != 4 or not 1 <= src.shape[3] <= 4 or min(src.shape) < 1 or H < 1 or W < 1:
        raise ValueError(f"undistort_host: src {src.dtype} {src.shape} -> {H}x{W} (expected uint8 (n, Hs, Ws, 1..4))")
    Hs, Ws = src.shape[1:3]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v, valid = source_map_host(model, params, k_out, Hs, Ws, xs, ys)
    uu, vv = np.where(valid, u, 0.0), np.where(valid, v, 0.0)
    x0 = np.minimum(np.floor(uu).astype(np.int64), Ws - 1)
    y0 = np.minimum(np.floor(vv).astype(np.int64), Hs - 1)
    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
    a, b = (uu - x0)[None, :, :, None], (vv - y0)[None, :, :, None]
    s = src.astype(np.float64)
    top = (1.0 - a) * s[:, y0, x0] + a * s[:, y0, x1]
    bot = (1.0 - a) * s[:, y1, x0] + a * s[:, y1, x1]
    val = np.where(valid[None, :, :, None], (1.0 - b) * top + b * bot, 0.0)
    out_valid = np.where(valid, 255, 0).astype(np.uint8) if want_valid else None
    return (val if unrounded else np.rint(val).astype(np.uint8)), out_valid


def border_valid(model, params, k_out, Hs, Ws, H, W):
    """True when every pixel on the border of the (H, W) output has a source."""
    xs = np.concatenate([np.arange(W), np.arange(W), np.zeros(H, np.int64), np.full(H, W - 1)])
    ys = np.concatenate([np.zeros(W, np.int64), np.full(W, H - 1), np.arange(H), np.arange(H)])
    return bool(source_map_host(model, params, k_out, Hs, Ws, xs, ys)[2].all())


def zoomed(K, z):
    """K with both focal lengths times z (the principal point stays)."""
    K = np.array(K, np.float64)
    K[0, 0], K[1, 1] = z * K[0, 0], z * K[1, 1]
    return K


def fit_zoom(model, params, K, Hs, Ws):
    """The smallest zoom z in [1, 4] (to the bisection's resolution, from above) for which the pinhole camera `zoomed(K, z)`
    at the source size sees no blank pixel on its border: 1 when that already holds for K itself, else 40 bisections on [1, 4]
    of that predicate, evaluated with the host form of the map, taking the upper end.  A longer focal length at the same size
    and principal point only ever crops, so the search needs the distortion alone and never its inverse.  ValueError when
    even z = 4 leaves blank border pixels."""
    ok = lambda z: border_valid(model, params, zoomed(K, z), Hs, Ws, Hs, Ws)  # noqa: E731
    if ok(1.0):
        return 1.0
    lo, hi = 1.0, ZOOM_MAX
    if not ok(hi):
        raise ValueError(f"a zoom of {ZOOM_MAX:g} still leaves blank pixels on the border of the undistorted picture")
    for _ in range(ZOOM_BISECTIONS):
        mid = 0.5 * (lo + hi)
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi


def undistort_images(images, camera, fit="inside", device="cuda"):
    """``images`` (n,Hs,Ws,C) uint8 host array, all taken by ``camera`` (a `colmap2mvsnet.Camera`) -> (dst (n,Hs,Ws,C) uint8,
    valid (Hs,Ws) uint8, K' (3,3), z), host arrays: the pictures as the pinhole camera K' = `zoomed(K, z)` of the same size
    sees them.  ``fit``: "keep" is z = 1, "inside" is `fit_zoom`, a number is a zoom found earlier.  On a GPU the pictures go
    through `ops.image_undistort_u8` in groups of at most 8; with ``device="cpu"`` the host form stands in and `ops` is never
    imported."""
    import torch

    from .colmap2mvsnet import intrinsic_of

    if isinstance(fit, str) and fit not in UNDISTORT_FITS:
        raise ValueError(f"fit {fit!r}: expected one of {', '.join(UNDISTORT_FITS)}, or a zoom")
    images = np.ascontiguousarray(images)
    if images.dtype != np.uint8 or images.ndim != 4:
        raise ValueError(f"undistort_images: images {images.dtype} {images.shape} (expected uint8 (n, Hs, Ws, C))")
    Hs, Ws = images.shape[1:3]
    name = model_name(camera.model)
    K = intrinsic_of(camera)
    z = fit_zoom(name, camera.params, K, Hs, Ws) if fit == "inside" else 1.0 if fit == "keep" else float(fit)
    Kz = zoomed(K, z)
    k_out = _k_out(Kz)
    device = torch.device(device)
    outs, valid = [], None
    for first in range(0, len(images), GROUP):
        group = images[first:first + GROUP]
        if device.type == "cuda":
            from . import ops

            with torch.cuda.device(device):
                d, m = ops.image_undistort_u8(torch.from_numpy(group).to(device), MODEL_IDS[name], camera.params, k_out, Hs, Ws,
                                              want_valid=valid is None)
                d, m = d.cpu().numpy(), (m.cpu().numpy() if m is not None else None)
        else:
            d, m = undistort_host(group, name, camera.params, k_out, Hs, Ws, want_valid=valid is None)
        outs.append(d)
        valid = m if valid is None else valid
    return np.concatenate(outs), valid, Kz, z
