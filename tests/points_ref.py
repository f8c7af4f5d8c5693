"""numpy float64 restatement of point-cloud rendering (include/ufr.h, "point-cloud rendering"; csrc/splat.hip): projection,
footprint, the key order of the depth test, the resolve and eye-dome lighting, with the kernels' expressions and summation
orders.  Written from the rule text, independently of the kernel: the depth test is a sort, not an atomic.  Plain on purpose.
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def normalised_k(K):
    """K / K[2,2] in float64 (what render_points hands the library)"""
    K = np.asarray(K, np.float64)[:3, :3]
    return K / K[2, 2]


def project(points, k, w2c, z_min=0.0):
    """(px, py, z32, keep): rounded pixel positions (float64, half to even), (float)c.z, and which points survive the tests that
    do not depend on the image (finite coordinates, c.z > z_min, finite pixel)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    k = np.asarray(k, np.float64)
    m = np.asarray(w2c, np.float64)
    with np.errstate(all="ignore"):
        c = [((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + m[i, 3] for i in range(3)]
        q = [(k[i, 0] * c[0] + k[i, 1] * c[1]) + k[i, 2] * c[2] for i in range(3)]
        px, py = np.rint(q[0] / q[2]), np.rint(q[1] / q[2])
        keep = np.isfinite(p).all(1) & (c[2] > z_min) & np.isfinite(px) & np.isfinite(py)
        z32 = c[2].astype(np.float32)
    return px, py, z32, keep


def footprint(r):
    """the (dx, dy) offsets with dx^2 + dy^2 <= r^2 + r"""
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r + r]


def key_image(points, k, w2c, H, W, radius=1, z_min=0.0):
    """(H,W) uint64: per pixel the smallest (float bits of c.z) << 32 | index over the points whose footprint covers it, all
    ones where there is none"""
    px, py, z32, keep = project(points, k, w2c, z_min)
    # the footprint reaches at most `radius` pixels: anything further out touches nothing (and need not fit an integer)
    keep &= (px >= -radius) & (px <= W - 1 + radius) & (py >= -radius) & (py <= H - 1 + radius)
    idx = np.nonzero(keep)[0]
    keys = (z32[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    ix, iy = px[idx].astype(np.int64), py[idx].astype(np.int64)
    img = np.full(H * W, EMPTY, np.uint64)
    for dx, dy in footprint(int(radius)):
        x, y = ix + dx, iy + dy
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        np.minimum.at(img, (y[ok] * W + x[ok]), keys[ok])
    return img.reshape(H, W)


def resolve(keys, n_points, colors=None, base_color=(1.0, 1.0, 1.0), background=(255, 255, 255), edl_strength=0.0, edl_radius=1):
    """dict of image (H,W,3) uint8, depth (H,W) float32 (0: empty), point_id (H,W) int32 (-1: empty) of a key image"""
    keys = np.asarray(keys, np.uint64)
    H, W = keys.shape
    on = keys != EMPTY
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    on &= idx < n_points
    depth = np.where(on, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    point_id = np.where(on, idx, -1).astype(np.int32)
    if colors is None:
        col = np.broadcast_to(255.0 * np.asarray(base_color, np.float32).astype(np.float64), (H, W, 3))
    else:
        col = np.asarray(colors, np.uint8).astype(np.float64)[np.where(on, idx, 0)]
    I = np.ones((H, W))
    if edl_strength > 0:
        d = int(edl_radius)
        with np.errstate(all="ignore"):
            lz = np.log2(depth.astype(np.float64))
        s = np.zeros((H, W))
        for sx, sy in ((-d, 0), (d, 0), (0, -d), (0, d)):            # (x - d, y), (x + d, y), (x, y - d), (x, y + d), in this order
            o = np.zeros((H, W))
            ys, xs = np.mgrid[0:H, 0:W]
            yn, xn = ys + sy, xs + sx
            inside = (yn >= 0) & (yn < H) & (xn >= 0) & (xn < W)
            yc, xc = np.clip(yn, 0, H - 1), np.clip(xn, 0, W - 1)
            ok = inside & on[yc, xc] & on
            o[ok] = np.maximum(0.0, lz[ok] - lz[yc, xc][ok])
            s = s + o
        shaded = s > 0
        I[shaded] = np.exp(-(edl_strength * s[shaded]) / 4.0)
    image = np.empty((H, W, 3), np.uint8)
    image[:] = np.asarray(background, np.uint8)
    image[on] = np.clip(np.rint(col * I[..., None]), 0, 255).astype(np.uint8)[on]          # np.rint: half to even
    return dict(image=image, depth=depth.astype(np.float32), point_id=point_id)


def render(points, k, w2c, H, W, colors=None, radius=1, z_min=0.0, **kw):
    """One frame.  ``k`` 3x3 already divided by k[2,2], ``w2c`` 4x4 float64."""
    n = len(np.asarray(points).reshape(-1, 3))
    return resolve(key_image(points, k, w2c, H, W, radius, z_min), n, colors=colors, **kw)


def render_points(points, K, c2ws, H, W, colors=None, radius=1, supersample=1, edl_radius=None, **kw):
    """The images ``render_trajectory.render_points`` documents: at supersample s the splat at s H x s W with the supersampled
    intrinsics, radius min(4, s radius + (s - 1)) and edl_radius defaulting to s, then raster_ref's box filter"""
    from raster_ref import downsample

    s = int(supersample)
    S = np.array([[s, 0, (s - 1) / 2], [0, s, (s - 1) / 2], [0, 0, 1]], np.float64)
    k = normalised_k(S @ np.asarray(K, np.float64)[:3, :3])
    c2ws = np.asarray(c2ws, np.float64).reshape(-1, 4, 4)
    frames = [render(points, k, np.linalg.inv(c), s * H, s * W, colors=colors, radius=min(4, s * radius + (s - 1)),
                     edl_radius=s if edl_radius is None else edl_radius, **kw)["image"] for c in c2ws]
    frames = np.stack(frames)
    return downsample(frames, s) if s > 1 else frames
