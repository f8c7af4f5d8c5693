"""numpy restatement of the depth-map fusion interface (uforecon_amd/depth_fusion.py, include/ufr.h ufr_depth_*): test
infrastructure, like chamfer_ref.py.  It follows the reference's code1/encoder_utils/depth_fusion.py operation by operation
and dtype by dtype, so that on the same numpy it gives the reference's bits (tests/test_depth_fusion.py checks that against
a recorded run of the reference).

``remap`` is a numpy statement of ``cv2.remap(src, x, y, interpolation=cv2.INTER_LINEAR)`` (constant border 0) as OpenCV's
source defines it for float32 maps (imgproc/src/imgwarp.cpp: the maps are converted to fixed point with INTER_BITS = 5,
``remapBilinear`` then blends four taps with a float table):
  * sx = round-half-even(x * 32) as int32; integer part ix = sx >> 5 (arithmetic) saturated to int16; fraction fx = (sx & 31) / 32
  * weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx*fy as float32 products, value = ((v00 w00 + v01 w01) + v10 w10) + v11 w11 in float32
  * a tap outside the image is 0, per tap
  * a non-finite coordinate, or one with |x * 32| >= 2^31, gives 0 (the x86 conversion gives INT_MIN: every tap outside)
No OpenCV was at hand when this was written: the statement is NOT compared with a real cv2.
"""
import numpy as np


def remap(src, x, y):
    src = np.asarray(src, np.float32)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    h, w = src.shape
    with np.errstate(invalid="ignore", over="ignore"):
        x32, y32 = x * np.float32(32), y * np.float32(32)
        good = (np.abs(x32) < np.float32(2.0 ** 31)) & (np.abs(y32) < np.float32(2.0 ** 31))      # False for NaN / inf
        sx = np.rint(np.where(good, x32, 0)).astype(np.int64)
        sy = np.rint(np.where(good, y32, 0)).astype(np.int64)
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    fx = (sx & 31).astype(np.float32) / np.float32(32)
    fy = (sy & 31).astype(np.float32) / np.float32(32)
    one = np.float32(1)

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], np.float32(0)).astype(np.float32)

    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((tap(ix, iy) * w00 + tap(ix + 1, iy) * w01) + tap(ix, iy + 1) * w10) + tap(ix + 1, iy + 1) * w11
    return np.where(good, v, np.float32(0)).astype(np.float32)


def taps_outside(src_shape, x, y):
    """how many of the four taps of ``remap`` fall outside an image of ``src_shape`` (4 for a non-finite coordinate)"""
    h, w = src_shape
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x32, y32 = x * np.float32(32), y * np.float32(32)
        good = (np.abs(x32) < np.float32(2.0 ** 31)) & (np.abs(y32) < np.float32(2.0 ** 31))
        ix = np.clip(np.rint(np.where(good, x32, 0)).astype(np.int64) >> 5, -32768, 32767)
        iy = np.clip(np.rint(np.where(good, y32, 0)).astype(np.int64) >> 5, -32768, 32767)
    n = np.zeros(x.shape, np.int32)
    for dx in (0, 1):
        for dy in (0, 1):
            n += ~((ix + dx >= 0) & (ix + dx < w) & (iy + dy >= 0) & (iy + dy < h))
    return np.where(good, n, 4)


def _grid(h, w):
    xs, ys = np.meshgrid(np.arange(0, w), np.arange(0, h))          # int64, as the reference's
    return xs, ys


def reproject(depth_ref, K_ref, E_ref, depth_src, K_src, E_src, sample=remap):
    """(depth_reprojected, x_reprojected, y_reprojected, x_src, y_src), float32 (H,W) each (depth_fusion.py:35-72)"""
    h, w = depth_ref.shape
    xs, ys = _grid(h, w)
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    ones = np.ones_like(xs)
    with np.errstate(all="ignore"):
        cam_ref = np.matmul(np.linalg.inv(K_ref), np.vstack((xs, ys, ones)) * depth_ref.reshape(-1))
        cam_src = np.matmul(np.matmul(E_src, np.linalg.inv(E_ref)), np.vstack((cam_ref, ones)))[:3]
        pix = np.matmul(K_src, cam_src)
        xy_src = pix[:2] / pix[2:3]
        x_src = xy_src[0].reshape(h, w).astype(np.float32)
        y_src = xy_src[1].reshape(h, w).astype(np.float32)
        sampled = sample(depth_src, x_src, y_src)
        cam_src = np.matmul(np.linalg.inv(K_src), np.vstack((xy_src, ones)) * sampled.reshape(-1))
        back = np.matmul(np.matmul(E_ref, np.linalg.inv(E_src)), np.vstack((cam_src, ones)))[:3]
        depth_rep = back[2].reshape(h, w).astype(np.float32)
        pix = np.matmul(K_ref, back)
        xy_rep = pix[:2] / (pix[2:3] + 1e-6)
        x_rep = xy_rep[0].reshape(h, w).astype(np.float32)
        y_rep = xy_rep[1].reshape(h, w).astype(np.float32)
    return depth_rep, x_rep, y_rep, x_src, y_src


def pair_check(depth_ref, K_ref, E_ref, depth_src, K_src, E_src, geo_pixel_thres, geo_depth_thres):
    """One pair (depth_fusion.py:75-90): dict of mask (bool), depth_reprojected (float32, 0 where not consistent), dist
    (float64), relative_depth_diff (float32), x_src, y_src."""
    h, w = depth_ref.shape
    xs, ys = _grid(h, w)
    depth_rep, x_rep, y_rep, x_src, y_src = reproject(depth_ref, K_ref, E_ref, depth_src, K_src, E_src)
    with np.errstate(all="ignore"):
        dist = np.sqrt((x_rep - xs) ** 2 + (y_rep - ys) ** 2)
        rel = np.abs(depth_rep - depth_ref) / depth_ref
        mask = np.logical_and(dist < geo_pixel_thres, rel < geo_depth_thres)
    depth_rep[~mask] = 0
    return dict(mask=mask, depth_reprojected=depth_rep, dist=dist, relative_depth_diff=rel, x_src=x_src, y_src=y_src)


def consistency(depth_ref, K_ref, E_ref, sources, geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2):
    """One reference view against ``sources`` = [(depth, K, E) ...] (depth_fusion.py:176-192): dict of pairs (the
    ``pair_check`` results), geo_mask_sum (int32), geo_mask (bool), depth_est_averaged (float64)."""
    pairs = [pair_check(depth_ref, K_ref, E_ref, d, K, E, geo_pixel_thres, geo_depth_thres) for d, K, E in sources]
    geo_mask_sum = 0
    for p in pairs:
        geo_mask_sum += p["mask"].astype(np.int32)
    averaged = (sum(p["depth_reprojected"] for p in pairs) + depth_ref) / (geo_mask_sum + 1)
    return dict(pairs=pairs, geo_mask_sum=geo_mask_sum, geo_mask=geo_mask_sum >= geo_mask_thres, depth_est_averaged=averaged)


def points(mask, depth_avg, color, K_ref, E_ref):
    """(xyz float32 (N,3), rgb uint8 (N,3)) of the pixels of ``mask`` in row-major order (depth_fusion.py:202-214, and the
    float32 narrowing of :219).  ``color`` (H,W,3) uint8: the reference's (img / 255.) * 255 truncates back to it."""
    h, w = mask.shape
    xs, ys = _grid(h, w)
    xs, ys, d = xs[mask], ys[mask], depth_avg[mask]
    cam = np.matmul(np.linalg.inv(K_ref), np.vstack((xs, ys, np.ones_like(xs))) * d)
    world = np.matmul(np.linalg.inv(E_ref), np.vstack((cam, np.ones_like(xs))))[:3]
    col = np.asarray(color, np.uint8)[mask]
    col = ((col.astype(np.float32) / 255.) * 255).astype(np.uint8)
    return world.transpose((1, 0)).astype(np.float32), col


def fuse_views(depths, intrinsics, extrinsics, colors, pairs, geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2):
    """The interface of uforecon_amd.depth_fusion.fuse_views with return_details=True, on the host."""
    out_xyz, out_rgb, masks, details = [], [], [], []
    for ref, srcs in pairs:
        r = consistency(depths[ref], intrinsics[ref], extrinsics[ref], [(depths[s], intrinsics[s], extrinsics[s]) for s in srcs],
                        geo_pixel_thres, geo_depth_thres, geo_mask_thres)
        xyz, rgb = points(r["geo_mask"], r["depth_est_averaged"], colors[ref], intrinsics[ref], extrinsics[ref])
        out_xyz.append(xyz)
        out_rgb.append(rgb)
        masks.append(r["geo_mask"])
        details.append(dict(geo_mask_sum=r["geo_mask_sum"], depth_est_averaged=r["depth_est_averaged"],
                            pair_masks=np.stack([p["mask"] for p in r["pairs"]]),
                            dist=np.stack([p["dist"] for p in r["pairs"]]),
                            relative_depth_diff=np.stack([p["relative_depth_diff"] for p in r["pairs"]])))
    xyz = np.concatenate(out_xyz) if out_xyz else np.zeros((0, 3), np.float32)
    rgb = np.concatenate(out_rgb) if out_rgb else np.zeros((0, 3), np.uint8)
    return xyz, rgb, masks, details


def close_pairs(dist, rel, geo_pixel_thres, geo_depth_thres):
    """the near-threshold (pair, pixel)s exempt from exact mask equality: about ten fp32 ulps of a coordinate below 2048
    (1.2e-4 px) and of a relative depth (6e-8)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(dist - geo_pixel_thres) < 1e-3) | (np.abs(rel.astype(np.float64) - geo_depth_thres) < 1e-5)
