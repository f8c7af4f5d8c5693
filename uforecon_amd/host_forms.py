"""The loaders' picture work: reading the files, the host forms of the picture and ray kernels of csrc/frame_input.hip, and the
calls that pick a kernel or its host form by device (`image_planes`, `pixel_rays`; the third, for the ground-truth depth maps
that only the training layout has, is `dtu_train.depth_gt`).

A loader computes per pixel on the device: the pictures through `ops.image_resize_u8` / `ops.image_resize_mask_u8`,
the ray tables through `ops.pixel_rays`.  With ``device="cpu"`` the host forms below stand in, and `ops` (so the native library)
is never imported.

Restated, not compared (no OpenCV was at hand; the rule written here is the rule):

  `resize_u8`  cv2.resize for 8-bit images with the default INTER_LINEAR: its fixed-point arithmetic as include/ufr.h
          (ufr_image_resize_u8) states it, the 2x2 box mean when both factors are exactly 2.
  `imread_gray`  a mask file with one channel (PIL mode "L") is read as it is; any other file is reduced with PIL's
          ``convert("L")``, the ITU-R 601-2 luma L = (299 R + 587 G + 114 B) / 1000 of its RGB form in PIL's integer arithmetic.
          cv2.imread(path, 0) decodes a colour JPEG straight to its luma plane and weighs a colour PNG with its own fixed-point
          constants, so a colour mask may differ from the reference's by a grey level; a single-channel mask does not.
"""
from __future__ import annotations

import numpy as np
import torch

from .cameras import homo_pixels


# ------------------------------------------------------------------ files
def imread_rgb(path):
    """An 8-bit image file as (H, W, 3) uint8 RGB (cv2.imread gives the same bytes in BGR order)."""
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def imread_gray(path):
    """A mask file as (H, W) uint8: see the module text."""
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im if im.mode == "L" else im.convert("L"), dtype=np.uint8)


# ------------------------------------------------------------------ OpenCV's resize, restated
def _taps(n_dst: int, n_src: int, along_x: bool):
    d = np.arange(n_dst, dtype=np.float64)
    scale = np.float64(n_src) / np.float64(n_dst)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    if along_x:                                    # a tap outside the row: the edge pixel with weight 1
        lo, hi = s < 0, s >= n_src - 1
        s[lo], f[lo] = 0, 0
        s[hi], f[hi] = n_src - 1, 0
    s0 = np.clip(s, 0, n_src - 1)
    s1 = np.clip(s + 1, 0, n_src - 1)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    w1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s0, s1, w0, w1


def resize_u8(image, size):
    """cv2.resize(image, (W, H)) for uint8 images (..., Hs, Ws, C): see the module text."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim < 3:
        raise ValueError(f"resize_u8: expected a uint8 array (..., H, W, C), got {img.dtype} {img.shape}")
    W, H = int(size[0]), int(size[1])
    Hs, Ws = img.shape[-3], img.shape[-2]
    if W < 1 or H < 1 or Hs < 1 or Ws < 1:
        raise ValueError(f"resize_u8: {Hs}x{Ws} -> {H}x{W}")
    v = img.astype(np.int32)
    if Hs == 2 * H and Ws == 2 * W:
        out = (v[..., 0::2, 0::2, :] + v[..., 0::2, 1::2, :] + v[..., 1::2, 0::2, :] + v[..., 1::2, 1::2, :] + 2) >> 2
        return out.astype(np.uint8)
    x0, x1, a0, a1 = _taps(W, Ws, True)
    y0, y1, b0, b1 = _taps(H, Hs, False)
    rows = v[..., :, x0, :] * a0[:, None] + v[..., :, x1, :] * a1[:, None]            # (..., Hs, W, C) int32
    r0, r1 = rows[..., y0, :, :], rows[..., y1, :, :]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


# ------------------------------------------------------------------ the host forms of the kernels
def image_planes_host(images, H: int, W: int, clip=(0, 0, 0, 0)):
    """ufr_image_resize_u8 on the host: (n,Hs,Ws,3) uint8 -> (n,3,Ho,Wo) float32 array, value = float32(double(v) / 255)."""
    images = np.asarray(images)
    H, W = int(H), int(W)
    left, top, right, bottom = (int(c) for c in clip)
    if images.ndim != 4 or images.shape[3] != 3 or min(left, top, right, bottom) < 0 or H - top - bottom < 1 or W - left - right < 1:
        raise ValueError(f"image_planes_host: images {images.shape}, {H}x{W}, clip {tuple(clip)}")
    small = resize_u8(images, (W, H)) / 255.
    small = small[:, top:H - bottom, left:W - right]
    return np.ascontiguousarray(np.transpose(small, (0, 3, 1, 2))).astype(np.float32)


def image_mask_planes_host(images, masks, H: int, W: int, clip=(0, 0, 0, 0)):
    """ufr_image_resize_mask_u8 on the host, in the reference's calls (general_fit.py:174-180): colour (n,Hs,Ws,3) and mask
    (n,Hs,Ws) uint8 each through `resize_u8`, value = float32((v / 255) * (m / 254)) with the product taken in float64."""
    images, masks = np.asarray(images), np.asarray(masks)
    H, W = int(H), int(W)
    left, top, right, bottom = (int(c) for c in clip)
    if images.ndim != 4 or images.shape[3] != 3 or masks.shape != images.shape[:3] or masks.dtype != np.uint8 \
            or min(left, top, right, bottom) < 0 or H - top - bottom < 1 or W - left - right < 1:
        raise ValueError(f"image_mask_planes_host: images {images.shape}, masks {masks.dtype} {masks.shape}, {H}x{W}, clip {tuple(clip)}")
    small = resize_u8(images, (W, H)) / 255.
    small = small * (resize_u8(masks[..., None], (W, H)) / 254.)
    small = small[:, top:H - bottom, left:W - right]
    return np.ascontiguousarray(np.transpose(small, (0, 3, 1, 2))).astype(np.float32)


def pixel_rays64(m_inv, homo_pixel, origin=None):
    """The reference's ray table in its own calls (dtu_test_sparse.py:423-429, dtu_train.py:473-478): the float32 matrix times
    the float64 pixel table in numpy, minus the origin, over torch.norm.  Returns a (3, H*W) float64 CPU tensor."""
    m = torch.as_tensor(m_inv, dtype=torch.float32)
    v = torch.from_numpy(np.matmul(m.numpy(), homo_pixel))[:3]          # what `tensor @ ndarray` evaluates
    if origin is not None:
        v = v - torch.as_tensor(origin, dtype=torch.float32)[:, None]
    return v / torch.norm(v, dim=0)


def pixel_rays_host(m_inv, H: int, W: int, origin=None, homo_pixel=None):
    """ufr_pixel_rays on the host: `pixel_rays64` cast to float32 at the end.  Returns a (3, H*W) CPU tensor."""
    if int(H) < 2 or int(W) < 2:
        raise ValueError(f"pixel_rays_host: image {H}x{W} (H and W must be >= 2)")
    return pixel_rays64(m_inv, homo_pixels(int(H), int(W)) if homo_pixel is None else homo_pixel, origin).float()


# ------------------------------------------------------------------ the kernel on a GPU, its host form on "cpu"
def image_planes(device, images, H: int, W: int, clip=(0, 0, 0, 0), masks=None):
    """(n,Hs,Ws,3) uint8 pictures (and (n,Hs,Ws) uint8 foreground masks) as host arrays -> (n,3,Ho,Wo) float32 on ``device``."""
    device = torch.device(device)
    if device.type == "cuda":
        from . import ops

        with torch.cuda.device(device):
            dev = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
            return ops.image_resize_u8(dev(images), H, W, clip) if masks is None else ops.image_resize_mask_u8(dev(images), dev(masks), H, W, clip)
    planes = image_planes_host(images, H, W, clip) if masks is None else image_mask_planes_host(images, masks, H, W, clip)
    return torch.from_numpy(planes).to(device)


def pixel_rays(device, m_inv, H: int, W: int, origin=None, homo_pixel=None):
    """The (3, H*W) float32 ray table on ``device``; ``m_inv`` 4x4 and ``origin`` (3 values or None) are CPU tensors."""
    device = torch.device(device)
    if device.type == "cuda":
        from . import ops

        with torch.cuda.device(device):
            return ops.pixel_rays(m_inv.numpy(), H, W, None if origin is None else origin.numpy(), device)
    return pixel_rays_host(m_inv, H, W, origin, homo_pixel).to(device)
