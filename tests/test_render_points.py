"""Point-cloud rendering and the DTU error clouds (uforecon_amd/render_trajectory.py's render_points, csrc/splat.hip,
uforecon_amd/dtu_eval.py's error_clouds), the parts that need no GPU: the numpy restatement of the kernels (points_ref.py) against
a brute-force loop over pixels and points, the header against the ctypes signatures, the command line's flags and defaults, the
colour rule of the error clouds against a restatement written here, and the coloured PLY writer against the reader."""
import math
import os
import re
import struct

import numpy as np
import torch

import points_ref as PR
from uforecon_amd import _lib, dtu_eval, render_trajectory as RT

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------ points_ref against a loop
def _f32_bits(z):
    return struct.unpack("<I", struct.pack("<f", z))[0]


def brute_force(points, k, w2c, H, W, radius, colors, background, edl_strength, edl_radius):
    """per pixel, per point, in python floats (IEEE double): the rule text of include/ufr.h read literally"""
    best = [[None] * W for _ in range(H)]                       # (depth as float32, index)
    for i, p in enumerate(points):
        c = [((w2c[r][0] * p[0] + w2c[r][1] * p[1]) + w2c[r][2] * p[2]) + w2c[r][3] for r in range(3)]
        if not all(math.isfinite(v) for v in p) or not c[2] > 0:
            continue
        q = [(k[r][0] * c[0] + k[r][1] * c[1]) + k[r][2] * c[2] for r in range(3)]
        px, py = round(q[0] / q[2]), round(q[1] / q[2])         # python's round: half to even
        z = float(np.float32(c[2]))
        for y in range(H):
            for x in range(W):
                dx, dy = x - px, y - py
                if dx * dx + dy * dy <= radius * radius + radius:
                    cand = (_f32_bits(z), i)
                    if best[y][x] is None or cand < best[y][x]:
                        best[y][x] = cand
    image = np.empty((H, W, 3), np.uint8)
    depth = np.zeros((H, W), np.float32)
    ids = np.full((H, W), -1, np.int32)
    zof = lambda b: struct.unpack("<f", struct.pack("<I", b[0]))[0]  # noqa: E731
    for y in range(H):
        for x in range(W):
            b = best[y][x]
            if b is None:
                image[y, x] = background
                continue
            z = zof(b)
            depth[y, x], ids[y, x] = z, b[1]
            s = 0.0
            for xn, yn in ((x - edl_radius, y), (x + edl_radius, y), (x, y - edl_radius), (x, y + edl_radius)):
                o = 0.0
                if 0 <= xn < W and 0 <= yn < H and best[yn][xn] is not None:
                    o = max(0.0, math.log2(z) - math.log2(zof(best[yn][xn])))
                s = s + o
            I = math.exp(-(edl_strength * s) / 4.0) if edl_strength > 0 and s > 0 else 1.0
            for ch in range(3):
                v = float(np.rint(float(colors[b[1]][ch]) * I))
                image[y, x, ch] = int(min(255.0, max(0.0, v)))
    return image, depth, ids


def small_scene():
    rng = np.random.default_rng(5)
    H, W, N = 7, 9, 40
    k = np.array([[6.0, 0.0, 4.0], [0.0, 6.0, 3.0], [0.0, 0.0, 1.0]])
    w2c = np.eye(4)
    w2c[:3, :3] = [[0.96, 0.0, 0.28], [0.0, 1.0, 0.0], [-0.28, 0.0, 0.96]]
    w2c[:3, 3] = [0.1, -0.05, 2.0]
    pts = rng.uniform(-1.2, 1.2, (N, 3))
    pts[:6, 2] = -4.0                                          # behind the camera
    pts[6] = pts[7]                                            # an exact duplicate: the lower index wins
    pts[8, 1] = np.nan
    pts[9, 0] = np.inf
    colors = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    return H, W, k, w2c, pts, colors


def test_points_ref_equals_a_brute_force_loop():
    H, W, k, w2c, pts, colors = small_scene()
    for radius, strength, d in ((0, 0.0, 1), (1, 0.0, 1), (2, 3.0, 1), (1, RT.DEFAULT_EDL, 2), (4, 1.0, 3)):
        got = PR.render(pts, k, w2c, H, W, colors=colors, radius=radius, background=(9, 8, 7), edl_strength=strength, edl_radius=d)
        image, depth, ids = brute_force(pts.tolist(), k.tolist(), w2c.tolist(), H, W, radius, colors.tolist(), (9, 8, 7), strength, d)
        assert np.array_equal(got["point_id"], ids), radius
        assert np.array_equal(got["depth"], depth), radius
        assert np.array_equal(got["image"], image), radius
        assert (ids >= 0).any() and ((ids < 0).any() or radius > 1)       # 40 discs of 21 pixels fill a 9 x 7 image
    assert not np.isin(np.arange(6), ids).any() and 7 not in ids and 8 not in ids and 9 not in ids


def test_footprint_sizes_and_base_colour():
    assert [len(PR.footprint(r)) for r in range(5)] == [1, 9, 21, 37, 69]
    H, W, k, w2c, pts, _ = small_scene()
    a = PR.render(pts, k, w2c, H, W, radius=1, base_color=(1.0, 0.5, 0.25))
    on = a["point_id"] >= 0
    assert on.any() and (a["image"][on] == [255, 128, 64]).all() and (a["image"][~on] == 255).all()    # 127.5 -> 128, 63.75 -> 64
    assert (a["depth"][~on] == 0).all() and (a["depth"][on] > 0).all()


# ------------------------------------------------------------------ header, signatures, command line
def test_header_section_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "ufr.h")).read()
    at = hdr.index("point-cloud rendering (ABI 507, additive)")
    assert at > hdr.index("mesh rendering (ABI 507, additive)")
    section = hdr[at:]
    end = section.find("/* ----", 10)
    section = section[:end if end > 0 else len(section)]
    declared = set(re.findall(r"\b(ufr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)))
    assert declared == {"ufr_splat_frames_workspace_bytes", "ufr_splat_frames"}
    assert declared <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["ufr_splat_frames"][1]) == 20 and len(_lib.SIGNATURES["ufr_splat_frames_workspace_bytes"][1]) == 2
    assert _lib.ABI_VERSION == 507 and "#define UFR_ABI_VERSION 507" in hdr


def test_parser_accepts_the_point_flags_and_keeps_every_default():
    p = RT.make_parser()
    d = vars(p.parse_args([]))
    assert d == dict(mesh_dir="./outputs/mesh/final", root_dir="./dtu_test", out_dir="./rendering", scans=dtu_eval.DTU_SCANS,
                     views=[23, 24, 23], num_views=240, img_wh=[800, 640], original_img_wh=[1600, 1200], offset_dist=25.0,
                     supersample=1, flat=False, color="uniform", ambient=0.25, format="jpg", quality=90, dump_poses=None,
                     pcd_dir=None, ply=None, point_radius=1, edl=RT.DEFAULT_EDL)
    a = p.parse_args(["--pcd_dir", "out/pcd", "--point_radius", "2", "--edl", "50", "--color", "vertex"])
    assert (a.pcd_dir, a.ply, a.point_radius, a.edl, a.color) == ("out/pcd", None, 2, 50.0, "vertex")
    a = p.parse_args(["--ply", "a/vis_024_d2s.ply", "b.ply", "--edl", "0"])
    assert a.ply == ["a/vis_024_d2s.ply", "b.ply"] and a.edl == 0.0 and a.pcd_dir is None
    assert RT.DEFAULT_EDL == 200
    assert abs(math.log(2) / (math.log2(1.01) / 4) - 193) < 0.5           # the derivation the constant is rounded from
    assert "not tuned" in " ".join(p.format_help().split())


# ------------------------------------------------------------------ error clouds
def hand_details():
    """12 data points (shuffled cloud), 9 ground-truth points, every mask by hand"""
    rng = np.random.default_rng(11)
    data_pcd = rng.normal(size=(12, 3)) * 50
    thin = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1], bool)            # 10 kept
    inbound = np.array([1, 1, 1, 0, 1, 1, 1, 1, 0, 1], bool)               # of the 10: 8
    grid_inbound = np.array([1, 1, 1, 1, 0, 1, 1, 1], bool)                # of the 8: 7
    in_obs = np.array([1, 0, 1, 1, 1, 1, 1], bool)                         # of the 7: 6
    max_dist, vis = 20.0, 10.0
    dist_d2s = np.array([0.0, vis, np.nextafter(max_dist, 0), max_dist, np.inf, 3.3])
    gt = rng.normal(size=(9, 3)) * 50
    above = np.array([1, 0, 1, 1, 1, 0, 1, 1, 1], bool)                    # 7
    dist_s2d = np.array([np.inf, 0.0, 2.5, vis, max_dist, np.nextafter(max_dist, 0), 0.02])
    t = torch.from_numpy
    details = dict(data_pcd=t(data_pcd), thin_mask=t(thin), inbound=t(inbound), grid_inbound=t(grid_inbound), in_obs=t(in_obs),
                   above=t(above), dist_d2s=t(dist_d2s), dist_s2d=t(dist_s2d))
    return details, gt, max_dist, vis


def numpy_error_colours(n, where, dist, max_dist, vis):
    col = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1))
    for j, i in enumerate(where):
        a = min(dist[j], vis) / vis
        col[i] = (0.0, 1.0, 0.0) if dist[j] >= max_dist else (1.0, 1.0 - a, 1.0 - a)
    return np.rint(255.0 * col).astype(np.uint8)


def test_error_clouds_equal_a_numpy_restatement():
    details, gt, max_dist, vis = hand_details()
    (dp, dc), (sp, sc) = dtu_eval.error_clouds(details, gt, max_dist=max_dist, vis_dist=vis)
    assert dp.dtype == torch.float64 and dc.dtype == torch.uint8 and sp.dtype == torch.float64 and sc.dtype == torch.uint8
    d = {k: v.numpy() for k, v in details.items()}
    down = d["data_pcd"][d["thin_mask"]]
    where = np.nonzero(d["inbound"])[0][d["grid_inbound"]][d["in_obs"]]
    assert np.array_equal(dp.numpy(), down) and np.array_equal(sp.numpy(), gt)
    want_d = numpy_error_colours(len(down), where, d["dist_d2s"], max_dist, vis)
    want_s = numpy_error_colours(len(gt), np.nonzero(d["above"])[0], d["dist_s2d"], max_dist, vis)
    assert np.array_equal(dc.numpy(), want_d) and np.array_equal(sc.numpy(), want_s)
    # the cases by hand: 0 -> white, vis_dist and just below max_dist -> red, max_dist and inf -> green, 3.3 -> 255 * 0.67 = 170.85
    assert dc.numpy()[where].tolist() == [[255, 255, 255], [255, 0, 0], [255, 0, 0], [0, 255, 0], [0, 255, 0], [255, 171, 171]]
    blue = (dc.numpy() == [0, 0, 255]).all(1)
    assert blue.sum() == len(down) - 6 and not blue[where].any()
    assert ((sc.numpy() == [0, 0, 255]).all(1) == ~d["above"]).all()
    assert sc.numpy()[np.nonzero(d["above"])[0][[0, 4]]].tolist() == [[0, 255, 0], [0, 255, 0]]


def test_coloured_ply_reads_back_bit_equal(tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(257, 3)) * 1e3
    pts[0] = [np.nextafter(1.0, 2.0), -0.0, 5e-324]                          # what a float writer would lose
    col = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    path = str(tmp_path / "vis_024_d2s.ply")
    dtu_eval.write_ply_points(path, pts, col)
    v, f, c = dtu_eval.read_ply(path, with_colors=True)
    assert f is None and v.dtype == np.float64 and c.dtype == np.uint8
    assert v.tobytes() == pts.tobytes() and np.array_equal(c, col)
    dtu_eval.write_ply_points(path, np.zeros((0, 3)), np.zeros((0, 3), np.uint8))
    v, f, c = dtu_eval.read_ply(path, with_colors=True)
    assert v.shape == (0, 3) and c.shape == (0, 3)
    assert open(path, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\n")
