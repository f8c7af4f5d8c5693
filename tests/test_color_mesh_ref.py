"""Mesh colouring (uforecon_amd/color_mesh.py, csrc/mesh_color.hip), the parts that need no GPU: known answers on the numpy
restatement (color_mesh_ref.py), the PLY writer, the parser's defaults and the command's one-line failures.  The scenes built
here (the two squares, the cut-off vertices, the two-angle vertex) are what test_gpu_color_mesh.py runs on the device against
the same known answers."""
import json
import os
import re

import numpy as np
import pytest

import color_mesh_ref as R
import raster_ref as RR
from uforecon_amd import clean_mesh as CM, color_mesh as CMesh, dtu_eval, ops

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILL = (7, 8, 9)


def grid_square(n, half, z, centre=(0.0, 0.0)):
    """an (n x n)-vertex square in the plane z = ``z``, 2 (n - 1)^2 faces"""
    xs = np.linspace(-half, half, n)
    v = np.array([(centre[0] + x, centre[1] + y, z) for y in xs for x in xs], np.float64)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [(a, a + 1, a + n), (a + 1, a + n + 1, a + n)]
    return v, np.asarray(f, np.int32)


def cameras_of(K, c2ws):
    k, w, c = zip(*[R.projection_camera(K, c2w) for c2w in c2ws])
    return np.stack(k), np.stack(w), np.stack(c)


def ref_depth(v, f, K, c2w, H, W):
    """the mesh's z-depth from one camera by the rendering restatement (float32 cameras, as the rasteriser takes them)"""
    k_inv = np.linalg.inv(np.asarray(K, np.float64) / K[2, 2]).astype(np.float32)
    return RR.render(v, f, k_inv, np.asarray(c2w, np.float32), H, W)["depth"]


# ------------------------------------------------------------------ the affine ramp
def ramp_scene():
    H = W = 32
    v, f = grid_square(7, 1.0, 5.0, centre=(0.037, -0.021))
    K = R.intrinsics(H, W, 10.0)
    c2w = np.eye(4)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([2 * xs + 3 * ys + 10, 5 * xs + 20, 7 * ys + 1], -1).astype(np.uint8)
    px = np.stack([10.0 * v[:, 0] / 5.0 + 15.5, 10.0 * v[:, 1] / 5.0 + 15.5], 1)
    want = np.stack([2 * px[:, 0] + 3 * px[:, 1] + 10, 5 * px[:, 0] + 20, 7 * px[:, 1] + 1], 1)
    interior = (np.abs(v[:, 0] - 0.037) < 0.99) & (np.abs(v[:, 1] + 0.021) < 0.99)
    return dict(v=v, f=f, K=K, c2w=c2w, img=img[None], want=want, interior=interior, H=H, W=W)


def check_ramp(colors, used, s):
    """Bilinear interpolation reproduces an affine picture: the sample is the ramp's value at the projection up to the
    roundings of the projection (2 divisions, 8 products and sums on values <= 32: below 1e-13 pixels, times a slope <= 7) and
    of the six operations of the sample (each half an ulp of a value <= 255: 2.9e-14).  Bound on |s - ramp|: 1e-11.  So the
    byte is rint(ramp) wherever the ramp is further than 1e-9 from a half-integer -- every interior vertex here."""
    want = s["want"]
    safe = (np.abs(want - np.floor(want) - 0.5) > 1e-9).all(1)
    sel = s["interior"] & safe
    assert sel.sum() == s["interior"].sum() == 25
    assert (used[sel] == 1).all()
    assert np.array_equal(colors[sel], np.rint(want[sel]).astype(np.uint8))


def test_affine_ramp_is_reproduced_exactly():
    s = ramp_scene()
    depth = ref_depth(s["v"], s["f"], s["K"], s["c2w"], s["H"], s["W"])[None]
    k, w, c = cameras_of(s["K"], [s["c2w"]])
    colors, used = R.vertex_colors(s["v"], RR.vertex_normals(s["v"], s["f"]), s["img"], depth, k, w, c, fill=FILL)
    check_ramp(colors, used, s)
    colors2, used2 = R.vertex_colors(s["v"], None, s["img"], None, k, w, c, fill=FILL)       # no occlusion, no angle: every vertex
    assert (used2 == 1).all() and np.array_equal(colors2[s["interior"]], colors[s["interior"]])


# ------------------------------------------------------------------ two squares
def two_squares_scene():
    """A far square at z = 6 and a small near square at z = 4 that hides the far one's centre from camera A (at the origin,
    looking along +z).  Camera B stands to the side, at (3, 0, 0), and sees the far centre past the near square: its ray to
    (0, 0, 6) crosses z = 4 at x = 1, the near square ends at 0.3.  A's picture is red, B's blue."""
    H, W = 48, 64
    far_v, far_f = grid_square(7, 1.5, 6.0)
    near_v, near_f = grid_square(3, 0.3, 4.0)
    v = np.concatenate([far_v, near_v])
    f = np.concatenate([far_f, near_f + len(far_v)])
    K = R.intrinsics(H, W, 40.0)
    c2ws = np.stack([np.eye(4), R.look_at((3.0, 0.0, 0.0), target=(0.0, 0.0, 6.0), up=(0.0, -1.0, 0.0))])
    imgs = np.zeros((2, H, W, 3), np.uint8)
    imgs[0, :, :, 0] = 200
    imgs[1, :, :, 2] = 200
    return dict(v=v, f=f, K=K, c2ws=c2ws, imgs=imgs, H=H, W=W, centre=24, other=8, kw=dict(depth_tol=0.1, power=0, fill=FILL))


def check_two_squares(occluded, free, s):
    """``occluded`` / ``free``: (colors, views_used) with the depth maps and with depth=None.  The tolerance 0.1 lets B's slanted
    view of the far square through (over 1 % of depth per pixel at this toy focal length) and still separates 6 from 4."""
    (co, uo), (cf, uf) = occluded, free
    i, j = s["centre"], s["other"]
    assert uo[i] == 1 and tuple(co[i]) == (0, 0, 200)                 # hidden from A: B's colour alone
    assert uf[i] == 2 and tuple(cf[i]) == (100, 0, 100)               # without depth maps A's picture bleeds through
    assert uo[j] == 2 and tuple(co[j]) == (100, 0, 100)               # (-1, -1, 6), clear of the near square: both see it


def test_two_squares_occlusion():
    s = two_squares_scene()
    depth = np.stack([ref_depth(s["v"], s["f"], s["K"], c, s["H"], s["W"]) for c in s["c2ws"]])
    k, w, c = cameras_of(s["K"], s["c2ws"])
    occluded = R.vertex_colors(s["v"], None, s["imgs"], depth, k, w, c, **s["kw"])
    free = R.vertex_colors(s["v"], None, s["imgs"], None, k, w, c, **s["kw"])
    check_two_squares(occluded, free, s)


# ------------------------------------------------------------------ weights and modes
def two_angle_scene():
    """One vertex at the origin with normal +z, seen from (0, 0, 5) (cos = 1) and from (3, 0, 4) (|e| = 5, cos = 4 / 5 = 0.8
    exactly as the kernel forms it).  Uniform pictures of 100 and 200."""
    H = W = 16
    K = R.intrinsics(H, W, 20.0)
    c2ws = np.stack([R.look_at((0.0, 0.0, 5.0), up=(0.0, 1.0, 0.0)), R.look_at((3.0, 0.0, 4.0), up=(0.0, 1.0, 0.0))])
    imgs = np.empty((2, H, W, 3), np.uint8)
    imgs[0], imgs[1] = 100, 200
    return dict(v=np.zeros((1, 3)), n=np.array([[0.0, 0.0, 1.0]]), K=K, c2ws=c2ws, imgs=imgs)


# (100 + 200) / 2 = 150;  (100 + 0.8 * 200) / 1.8 = 144.4;  (100 + 0.64 * 200) / 1.64 = 139.02;  best: the frontal view
TWO_ANGLE_ANSWERS = [(0, "mean", 150), (1, "mean", 144), (2, "mean", 139), (1, "best", 100), (2, "best", 100), (0, "best", 100)]


@pytest.mark.parametrize("power,mode,want", TWO_ANGLE_ANSWERS)
def test_power_and_mode_hand_values(power, mode, want):
    s = two_angle_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    colors, used = R.vertex_colors(s["v"], s["n"], s["imgs"], None, k, w, c, power=power, mode=mode, min_cos=0.0)
    assert used[0] == 2 and tuple(colors[0]) == (want,) * 3


def test_best_mode_tie_goes_to_the_lowest_view():
    s = two_angle_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"][::-1])
    colors, _ = R.vertex_colors(s["v"], s["n"], s["imgs"][::-1], None, k, w, c, power=0, mode="best", min_cos=0.0)
    assert tuple(colors[0]) == (200,) * 3                              # equal weights: the first listed, now the 200 picture
    colors, _ = R.vertex_colors(s["v"], s["n"], s["imgs"][::-1], None, k, w, c, power=1, mode="best", min_cos=0.0)
    assert tuple(colors[0]) == (100,) * 3                              # unequal: the frontal one, wherever it stands


# ------------------------------------------------------------------ cut-offs
def cutoff_scene():
    """An identity camera with K = [[2, 0, 0], [0, 2, 0], [0, 0, 1]] and vertices at z = 2: (X, Y, 2) projects to the pixel
    (X, Y) exactly.  8 x 6 noise picture.  Returns the vertices, and per vertex the expected views_used and, where it is a
    known answer, the colour."""
    H, W = 6, 8
    img = np.random.default_rng(11).integers(0, 256, (1, H, W, 3)).astype(np.uint8)
    cases = [((3.0, 2.0, -2.0), 0, FILL),                      # behind the camera
             ((-0.5, 2.0, 2.0), 0, FILL),                      # x0 = -1: one pixel out on the left
             ((0.0, 2.0, 2.0), 1, tuple(img[0, 2, 0])),        # x0 = 0, on a pixel centre
             ((6.5, 2.0, 2.0), 1, None),                       # x0 + 1 == W - 1: the last footprint inside
             ((7.0, 2.0, 2.0), 0, FILL),                       # x0 + 1 == W: one pixel out on the right, though x itself is inside
             ((3.0, -0.5, 2.0), 0, FILL),                      # y0 = -1: out at the top
             ((3.0, 4.5, 2.0), 1, None),                       # y0 + 1 == H - 1
             ((3.0, 5.0, 2.0), 0, FILL),                       # y0 + 1 == H: out at the bottom
             ((3.0, 2.0, 2.0), 1, tuple(img[0, 2, 3])),        # fx = fy = 0: the texel itself
             ((np.nan, 2.0, 2.0), 0, FILL),                    # a NaN vertex
             ((3.0, np.inf, 2.0), 0, FILL)]
    v = np.array([c[0] for c in cases], np.float64)
    K = np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]])
    return dict(v=v, K=K, c2ws=np.eye(4)[None], img=img, used=[c[1] for c in cases], colors=[c[2] for c in cases])


def check_cutoffs(colors, used, s):
    assert used.tolist() == s["used"]
    for i, want in enumerate(s["colors"]):
        if want is not None:
            assert tuple(int(x) for x in colors[i]) == tuple(int(x) for x in want), i
    img = s["img"][0].astype(np.float64)
    assert tuple(colors[3]) == tuple(np.rint(0.5 * img[2, 6] + 0.5 * img[2, 7]).astype(np.uint8))      # half-way: exact in fp64
    assert tuple(colors[6]) == tuple(np.rint(0.5 * img[4, 3] + 0.5 * img[5, 3]).astype(np.uint8))


def test_cutoffs():
    s = cutoff_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    colors, used = R.vertex_colors(s["v"], None, s["img"], None, k, w, c, fill=FILL)
    check_cutoffs(colors, used, s)


def test_zero_normal_is_never_seen_and_min_cos_exactly_met_counts():
    s = two_angle_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    colors, used = R.vertex_colors(s["v"], np.zeros((1, 3)), s["imgs"], None, k, w, c, min_cos=0.0, fill=FILL)
    assert used[0] == 0 and tuple(colors[0]) == FILL
    colors, used = R.vertex_colors(s["v"], s["n"], s["imgs"], None, k, w, c, min_cos=0.8, power=0)
    assert used[0] == 2 and tuple(colors[0]) == (150,) * 3             # cos = 0.8 >= 0.8 counts
    colors, used = R.vertex_colors(s["v"], s["n"], s["imgs"], None, k, w, c, min_cos=np.nextafter(0.8, 1.0), power=0)
    assert used[0] == 1 and tuple(colors[0]) == (100,) * 3


# ------------------------------------------------------------------ fill
def strip(n):
    """a strip of n triangles (i, i + 1, i + 2) over n + 2 vertices: vertex i touches i - 2 .. i + 2"""
    return np.array([(i, i + 1, i + 2) for i in range(n)], np.int32)


def test_fill_advances_one_edge_per_round():
    f = strip(9)
    V = 11
    colors = np.full((V, 3), FILL, np.uint8)
    colors[0] = (10, 20, 30)
    used = np.zeros(V, np.uint8)
    used[0] = 1
    dist = (np.arange(V) + 1) // 2                                      # edges from vertex 0 along the strip
    for r in range(0, 7):
        c, st, run = R.fill(f, colors, used, r)
        assert np.array_equal(st != 0, dist <= r), r
        assert (c[st != 0] == (10, 20, 30)).all() and (c[st == 0] == FILL).all()
        assert run == min(r, 6)                                          # 5 rounds fill, the sixth finds nothing and is the last


def test_fill_counts_a_shared_neighbour_twice_and_rounds_half_to_even():
    f = np.array([(0, 1, 2), (0, 2, 3)], np.int32)
    colors = np.array([(0, 0, 0), (10, 1, 0), (40, 2, 1), (10, 3, 0)], np.uint8)
    used = np.array([0, 1, 1, 1], np.uint8)
    c, st, _ = R.fill(f, colors, used, 1)
    assert tuple(c[0]) == (25, 2, 0) and st[0] == 1       # (10 + 40 + 40 + 10) / 4, not 60 / 3; 8 / 4; 2 / 4 = 0.5 -> 0
    f1 = np.array([(0, 1, 2)], np.int32)
    colors = np.array([(0, 0, 0), (1, 2, 0), (2, 3, 1)], np.uint8)
    c, _, _ = R.fill(f1, colors, np.array([0, 1, 1], np.uint8), 1)
    assert tuple(c[0]) == (2, 2, 0)                        # 1.5 -> 2, 2.5 -> 2, 0.5 -> 0


def test_fill_leaves_an_isolated_vertex_empty():
    f = np.array([(0, 1, 2)], np.int32)
    colors = np.array([(5, 5, 5), FILL, FILL, FILL], np.uint8)
    c, st, run = R.fill(f, colors, np.array([1, 0, 0, 0], np.uint8), 10)
    assert st.tolist() == [1, 1, 1, 0] and tuple(c[3]) == FILL and run == 2


# ------------------------------------------------------------------ host code
def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    v, f = R.icosphere(1)
    v32 = v.astype(np.float32)
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    normals = rng.standard_normal((len(v), 3)).astype(np.float32)
    p = str(tmp_path / "a.ply")
    CMesh.write_ply(p, v32, f, colors)
    rv, rf, rc = dtu_eval.read_ply(p, with_colors=True)
    assert np.array_equal(rv.astype(np.float32), v32) and np.array_equal(rf, f) and np.array_equal(rc, colors) and rc.dtype == np.uint8
    CMesh.write_ply(p, v32, f, colors, normals=normals)
    rv, rf, rc, rn = dtu_eval.read_ply(p, with_colors=True, with_normals=True)
    assert np.array_equal(rv.astype(np.float32), v32) and np.array_equal(rf, f) and np.array_equal(rc, colors)
    assert np.array_equal(rn.astype(np.float32), normals)
    with pytest.raises(ValueError):
        CMesh.write_ply(p, v32, f, colors.astype(np.int32))


def test_parser_defaults():
    a = CMesh.make_parser().parse_args([])
    assert a.depth_tol == 0.005 and a.min_cos == 0.2 and a.power == 2 and a.fill_rounds == 8 and a.fill_color == [128, 128, 128]
    assert a.mode == "mean" and not a.no_occlusion and not a.all_views and a.views == CM.TEST_REF_VIEW
    assert a.scans == dtu_eval.DTU_SCANS and a.ply is None
    assert CMesh.make_parser().parse_args(["--all_views"]).all_views and CMesh.ALL_VIEWS == list(range(49))
    with pytest.raises(SystemExit):
        CMesh.make_parser().parse_args(["--all_views", "--views", "1"])
    import inspect

    sig = inspect.signature(ops.mesh_vertex_colors).parameters
    assert (sig["depth_tol"].default, sig["min_cos"].default, sig["power"].default) == (CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER)


def test_block_size_constant_matches_the_kernel():
    code = open(os.path.join(ROOT, "uforecon_amd", "csrc", "ufr_internal.h")).read()
    assert re.search(r"constexpr int kColorThreads = (\d+);", code).group(1) == str(ops.MESH_COLOR_BLOCK)
    hdr = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert "#define UFR_MESH_COLOR_MAX_POWER %d" % ops.MESH_COLOR_MAX_POWER in hdr
    assert "#define UFR_MESH_COLOR_MEAN 0" in hdr and "#define UFR_MESH_COLOR_BEST 1" in hdr and ops.MESH_COLOR_MODES == {"mean": 0, "best": 1}


def test_lib_signatures_match_the_header():
    import ctypes as C

    from uforecon_amd import _lib
    from uforecon_amd.build import SOURCES

    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert "mesh colouring (ABI 507, additive)" in text and "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = []
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_color_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        found.append(name)
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is (C.c_size_t if res == "size_t" else C.c_int), name
        want = [p.strip() for p in params.split(",")]
        assert len(want) == len(args), name
        for p, a in zip(want, args):
            if "*" in p or p.startswith("ufr_stream"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}[p.split()[0]], (name, p)
    assert sorted(found) == ["ufr_color_fill_round", "ufr_color_vertices", "ufr_color_vertices_workspace_bytes"]
    assert sorted(found) == sorted(n for n in _lib.SIGNATURES if n.startswith("ufr_color_"))
    assert "mesh_color.hip" in SOURCES


def test_command_failures_are_one_line_each(tmp_path, capsys):
    root, mesh_dir, out_dir = str(tmp_path / "dtu"), str(tmp_path / "mesh"), str(tmp_path / "out")
    os.makedirs(mesh_dir)
    v, f = R.icosphere(0)
    H, W = 6, 8
    rng = np.random.default_rng(0)
    pics = {s: [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)] for s in (1, 2, 3, 4)}
    pics[3][1] = rng.integers(0, 256, (H + 2, W, 3)).astype(np.uint8)
    R.write_dtu_tree(root, [1, 2, 3, 4], [5, 6], R.intrinsics(H, W, 10.0), R.ring_cameras(2, 4.0), pics)
    for s in (1, 2, 3):
        CM.write_ply(os.path.join(mesh_dir, "scan%d.ply" % s), v, f)
    CM.write_ply(os.path.join(mesh_dir, "scan4.ply"), v, np.zeros((0, 3), np.int32))
    os.remove(os.path.join(root, "scan1", "image", "000006.png"))
    common = ["--mesh_dir", mesh_dir, "--root_dir", root, "--out_dir", out_dir]
    assert CMesh.main(common + ["--scans", "1", "3", "4", "9", "--views", "5", "6"]) == 0
    assert CMesh.main(common + ["--scans", "2", "--views", "5", "7"]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 5
    assert lines[0].startswith("scan1: no picture at ") and lines[0].endswith("000006.png")
    assert lines[1].startswith("scan3: pictures of unequal size")
    assert lines[2].startswith("scan4: ") and lines[2].endswith("has no faces")
    assert lines[3].startswith("scan9: no mesh at ")
    assert lines[4].startswith("scan2: no camera at ") and lines[4].endswith("00000007_cam.txt")
    assert json.load(open(os.path.join(out_dir, "color_mesh.json"))) == {}
    assert not [p for p in os.listdir(out_dir) if p.endswith(".ply")]
