"""ufr_image_undistort_u8 as include/ufr.h states it, one pixel at a time in plain Python (`math`, Python floats: IEEE double,
every operation rounded on its own).  Written from the header, not from uforecon_amd/undistort.py: the tests hold the host
form (numpy) and, through it, the kernel against this."""
import math

# COLMAP's model ids and parameter lists, as the header gives them
MODELS = {"SIMPLE_PINHOLE": (0, ("f", "cx", "cy")), "PINHOLE": (1, ("fx", "fy", "cx", "cy")),
          "SIMPLE_RADIAL": (2, ("f", "cx", "cy", "k1")), "RADIAL": (3, ("f", "cx", "cy", "k1", "k2")),
          "OPENCV": (4, ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")),
          "OPENCV_FISHEYE": (5, ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4")),
          "FULL_OPENCV": (6, ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")),
          "SIMPLE_RADIAL_FISHEYE": (8, ("f", "cx", "cy", "k1")), "RADIAL_FISHEYE": (9, ("f", "cx", "cy", "k1", "k2"))}
POLYNOMIAL = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV")
FISHEYE = ("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")


def named(model, params):
    """{parameter name: value}, a coefficient the model does not have being 0; fx = fy = f for a one-focal model"""
    names = MODELS[model][1]
    assert len(names) == len(params), (model, len(params))
    p = {k: 0.0 for k in ("k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2")}
    p.update({k: float(v) for k, v in zip(names, params)})
    if "f" in p:
        p["fx"] = p["fy"] = p["f"]
    return p


def distort(model, params, x, y):
    p = named(model, params)
    xx, yy = x * x, y * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    xy = x * y
    if model in FISHEYE:
        r = math.sqrt(r2)
        t = math.atan(r)
        t2 = t * t
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t4 * t4
        s = 1.0 if r < 1e-8 else (t * ((((1 + (p["k1"] * t2)) + (p["k2"] * t4)) + (p["k3"] * t6)) + (p["k4"] * t8))) / r
        return x * s, y * s
    tx = ((2 * p["p1"]) * xy) + (p["p2"] * (r2 + (2 * xx)))
    ty = ((2 * p["p2"]) * xy) + (p["p1"] * (r2 + (2 * yy)))
    if model == "FULL_OPENCV":
        rad = (((1 + (p["k1"] * r2)) + (p["k2"] * r4)) + (p["k3"] * r6)) / (((1 + (p["k4"] * r2)) + (p["k5"] * r4)) + (p["k6"] * r6))
        return (x * rad) + tx, (y * rad) + ty
    assert model in POLYNOMIAL
    rad = (p["k1"] * r2) + (p["k2"] * r4)
    return (x + (x * rad)) + tx, (y + (y * rad)) + ty


def source_of(model, params, k_out, x, y):
    """(u, v): where the centre of output pixel (x, y) lies in the source picture, in pixel indices"""
    p = named(model, params)
    fxo, fyo, cxo, cyo = (float(k) for k in k_out)
    xn = ((x + 0.5) - cxo) / fxo
    yn = ((y + 0.5) - cyo) / fyo
    xd, yd = distort(model, params, xn, yn)
    return ((p["fx"] * xd) + p["cx"]) - 0.5, ((p["fy"] * yd) + p["cy"]) - 0.5


# cameras for a 9 x 7 source picture and the 8 x 6 output K_SMALL looks at, distorted enough that some output pixels have no source
K_SMALL = (5.5, 5.25, 4.1, 3.2)
SMALL_CAMERAS = {
    "SIMPLE_PINHOLE": (6.0, 4.4, 3.6),
    "PINHOLE": (6.0, 6.5, 4.4, 3.6),
    "SIMPLE_RADIAL": (6.0, 4.4, 3.6, 0.35),
    "RADIAL": (6.0, 4.4, 3.6, 0.3, 0.12),
    "OPENCV": (6.0, 6.5, 4.4, 3.6, 0.28, 0.09, 0.04, -0.03),
    "FULL_OPENCV": (6.0, 6.5, 4.4, 3.6, 0.3, 0.1, 0.02, -0.03, 0.05, 0.1, 0.02, 0.01),
    "OPENCV_FISHEYE": (6.0, 6.5, 4.4, 3.6, 0.6, 0.2, 0.05, 0.01),
    "SIMPLE_RADIAL_FISHEYE": (6.0, 4.4, 3.6, 0.9),
    "RADIAL_FISHEYE": (6.0, 4.4, 3.6, 0.7, 0.3),
}
TIE = 1e-9


def tie_pixels(val, u, v, Hs, Ws):
    """(near_half (n,H,W,C), near_bound (H,W)) bool arrays: where the unrounded value lies within TIE of a half-integer, and where
    u or v lies within TIE of a bound of the source picture -- the only places where two math libraries whose atan differs in the
    last place may disagree by one level, or on `valid`."""
    import numpy as np

    near_half = np.abs((val - np.floor(val)) - 0.5) < TIE
    with np.errstate(invalid="ignore"):
        near_bound = (np.abs(u) < TIE) | (np.abs(u - (Ws - 1)) < TIE) | (np.abs(v) < TIE) | (np.abs(v - (Hs - 1)) < TIE)
    return near_half, near_bound


def assert_same(got, want, ties=None):
    """(dst, valid) twice.  Without ``ties`` bytes and valid are equal; with ``ties`` = `tie_pixels(...)` of the host form they
    may differ by one level at a near-half value and on `valid` at a near-bound position, and nowhere else."""
    import numpy as np

    (dst, valid), (want_dst, want_valid) = (tuple(np.asarray(a) for a in pair) for pair in (got, want))
    assert dst.shape == want_dst.shape and valid.shape == want_valid.shape and dst.dtype == valid.dtype == np.uint8
    if ties is None:
        assert np.array_equal(valid, want_valid), int((valid != want_valid).sum())
        assert np.array_equal(dst, want_dst), int((dst != want_dst).sum())
        return
    near_half, near_bound = ties
    assert not ((valid != want_valid) & ~near_bound).any()
    both = ((valid == 255) & (want_valid == 255))[None, :, :, None]
    diff = np.abs(dst.astype(np.int64) - want_dst.astype(np.int64))
    assert not (both & (diff > 1)).any() and not (both & (diff == 1) & ~near_half).any(), int((both & (diff > 0)).sum())
    assert not (dst[:, valid == 0] != 0).any()


def round_half_even(val):
    lo = math.floor(val)
    d = val - lo
    return lo + 1 if d > 0.5 or (d == 0.5 and lo % 2 == 1) else lo


def undistort(src, model, params, k_out, H, W):
    """src: nested lists / an array [n][Hs][Ws][C] of ints -> (dst [n][H][W][C], valid [H][W], val [n][H][W][C] unrounded,
    uv [H][W] = (u, v)), nested lists"""
    n, Hs, Ws, C = len(src), len(src[0]), len(src[0][0]), len(src[0][0][0])
    dst = [[[[0] * C for _ in range(W)] for _ in range(H)] for _ in range(n)]
    val = [[[[0.0] * C for _ in range(W)] for _ in range(H)] for _ in range(n)]
    valid = [[0] * W for _ in range(H)]
    uv = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            u, v = source_of(model, params, k_out, x, y)
            uv[y][x] = (u, v)
            if not (0 <= u <= Ws - 1 and 0 <= v <= Hs - 1):          # a NaN fails the chain
                continue
            valid[y][x] = 255
            x0 = min(math.floor(u), Ws - 1)
            x1 = min(x0 + 1, Ws - 1)
            y0 = min(math.floor(v), Hs - 1)
            y1 = min(y0 + 1, Hs - 1)
            a, b = u - x0, v - y0
            for i in range(n):
                for c in range(C):
                    top = ((1 - a) * int(src[i][y0][x0][c])) + (a * int(src[i][y0][x1][c]))
                    bot = ((1 - a) * int(src[i][y1][x0][c])) + (a * int(src[i][y1][x1][c]))
                    val[i][y][x][c] = ((1 - b) * top) + (b * bot)
                    dst[i][y][x][c] = round_half_even(val[i][y][x][c])
    return dst, valid, val, uv
