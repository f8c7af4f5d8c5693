"""float64 forms of what a validation frame is scored and saved with (code1/model.py:708-726, :731-742), for the tests of
ufr_frame_metrics / ufr_frame_preview_u8 and of validation_step."""
from __future__ import annotations

import numpy as np

KEYS = ("val/loss_rgb_coarse", "val/loss_rgb_fine", "psnr/coarse", "psnr/fine", "val/loss_depth_coarse", "val/loss_depth_fine")


def _np(t, dtype=np.float64):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t).astype(dtype)


def psnr(x, y):
    """piq.psnr(clamp(x), clamp(y), data_range=1) restated: -10 log10(mean((x - y)^2) + 1e-8)."""
    d = np.clip(x, 0.0, 1.0) - np.clip(y, 0.0, 1.0)
    return -10.0 * np.log10(np.mean(d * d) + 1e-8)


def frame_metrics(rgb_c, rgb_f, rgb_gt, depth_c, depth_f, depth_gt, near, far):
    """The eight values of ufr_frame_metrics in float64.  rgb_c / rgb_f (n,3); rgb_gt (3,n) planar; depths (n)."""
    rgb_c, rgb_f = _np(rgb_c).reshape(-1, 3), _np(rgb_f).reshape(-1, 3)
    gt = _np(rgb_gt).reshape(3, -1).T
    dc, df, dg = _np(depth_c).reshape(-1), _np(depth_f).reshape(-1), _np(depth_gt).reshape(-1)
    near, far = np.float64(np.float32(near)), np.float64(np.float32(far))
    with np.errstate(invalid="ignore"):
        mask = (dg != 0) & (dg >= near) & (dg <= far)
    count = int(mask.sum())
    l1_c = float(np.mean(np.abs(dc[mask] - dg[mask]))) if count else 0.0
    l1_f = float(np.mean(np.abs(df[mask] - dg[mask]))) if count else 0.0
    return np.array([np.mean((rgb_c - gt) ** 2), np.mean((rgb_f - gt) ** 2), psnr(rgb_c, gt), psnr(rgb_f, gt), l1_c, l1_f,
                     float(count), np.max(dc)], dtype=np.float64)


def preview_u8(rgb, depth, scale):
    """model.py:731, :734, :742 in numpy's float32: (rgb8, depth8)."""
    rgb8 = (_np(rgb, np.float32).astype(np.float32) * 255).astype(np.uint8)
    depths = _np(depth, np.float32) * np.float32(scale)
    depth8 = ((depths / np.max(depths)).astype(np.float32) * 255).astype(np.uint8)
    return rgb8, depth8


def read_depth(pfm_rows, bottom_up, y0, x0, H, W, scale_factor, cam_ray_d_z):
    """dtu_train.py:249-254 (read_pfm's flip, the nearest half-size resize, the crop), :429 (x scale_factor in float32) and
    :485 (/ cam_ray_d.z) on the (Hs,Ws) rows as the file stores them; cam_ray_d_z (H*W) float32."""
    data = np.asarray(pfm_rows, np.float32)
    if bottom_up:
        data = np.flipud(data)
    half = data[0::2, 0::2]                       # INTER_NEAREST at fx = fy = 0.5: source pixel (2y, 2x)
    crop = half[y0:y0 + H, x0:x0 + W]
    scaled = (crop * np.float32(scale_factor)).astype(np.float32)
    return (scaled.reshape(-1) / np.asarray(cam_ray_d_z, np.float32).reshape(-1)).astype(np.float32).reshape(H, W)
