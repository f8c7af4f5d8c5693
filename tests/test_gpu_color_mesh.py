"""The mesh-colouring kernels (csrc/mesh_color.hip) against the numpy restatement (color_mesh_ref.py) on the device: colours,
views_used, fill states and round counts bit for bit -- both sides form the same float64 expressions without contraction, and
the depth maps the restatement is given are the device's own (``ops.raster_frames``).  Then the known answers of
test_color_mesh_ref.py on the device, a round trip through the rasteriser, the argument errors and the command."""
import json
import os

import numpy as np
import pytest

import color_mesh_ref as R
from test_color_mesh_ref import (FILL, TWO_ANGLE_ANSWERS, cameras_of, check_cutoffs, check_ramp, check_two_squares, cutoff_scene,
                                 ramp_scene, two_angle_scene, two_squares_scene)
from uforecon_amd import clean_mesh as CM, color_mesh as CMesh, dtu_eval, ops, render_trajectory as RT
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

H, W, FOCAL, DIST = 48, 64, 80.0, 4.0
BLOCK = ops.MESH_COLOR_BLOCK            # the vertices one block of the colour kernel owns: 256


def cuda(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def gpu_depth(v, f, K, c2ws, h, w):
    """(n,h,w) float32: the mesh's z-depth from every camera, one call per view as color_mesh makes them"""
    tv, tf = cuda(np.asarray(v, np.float64)), cuda(np.asarray(f, np.int32))
    out = []
    for c2w in c2ws:
        k_inv, c32 = CM.ray_camera(K.astype(np.float32), np.linalg.inv(c2w).astype(np.float32))
        out.append(ops.raster_frames(tv, tf, k_inv, c32[None], h, w, return_depth=True)["depth"][0].cpu().numpy())
    return np.stack(out)


def gpu_colors(v, n, imgs, depth, k, w, c, **kw):
    col, used = ops.mesh_vertex_colors(cuda(np.asarray(v, np.float64)), None if n is None else cuda(np.asarray(n, np.float64)),
                                       cuda(imgs), None if depth is None else cuda(depth), k, w, c, **kw)
    return col.cpu().numpy(), used.cpu().numpy()


_scenes = {}


def sphere_scene(n_views):
    """the 642-vertex icosphere, ``n_views`` ring cameras, noise pictures and the device's depth maps; built once per view
    count and shared (never modified)"""
    if n_views not in _scenes:
        v, f = R.icosphere(3)
        normals = ops.raster_vertex_normals(cuda(v), cuda(f)).cpu().numpy()
        K = R.intrinsics(H, W, FOCAL)
        c2ws = R.ring_cameras(n_views, DIST, height=0.7)
        imgs = np.random.default_rng(100 + n_views).integers(0, 256, (n_views, H, W, 3)).astype(np.uint8)
        k, w, c = cameras_of(K, c2ws)
        _scenes[n_views] = dict(v=v, f=f, n=normals, imgs=imgs, depth=gpu_depth(v, f, K, c2ws, H, W), k=k, w=w, c=c)
    return _scenes[n_views]


def assert_bits(s, V=None, occlusion=True, **kw):
    V = len(s["v"]) if V is None else V
    kw = dict(dict(depth_tol=0.02, fill=FILL), **kw)
    depth = s["depth"] if occlusion else None
    got = gpu_colors(s["v"][:V], s["n"][:V], s["imgs"], depth, s["k"], s["w"], s["c"], **kw)
    want = R.vertex_colors(s["v"][:V], s["n"][:V], s["imgs"], depth, s["k"], s["w"], s["c"], **kw)
    print(f"V {V}: seen {(want[1] > 0).sum()}, views_used histogram {np.bincount(want[1]).tolist()}, "
          f"colour mismatches {(got[0] != want[0]).any(1).sum()}, views_used mismatches {(got[1] != want[1]).sum()}")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    return got


# ------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("mode", ["mean", "best"])
@pytest.mark.parametrize("occlusion", [True, False])
def test_three_views_match_the_restatement_and_repeat(mode, occlusion):
    s = sphere_scene(3)
    got = assert_bits(s, mode=mode, occlusion=occlusion)
    seen = got[1] > 0
    assert 0.3 < seen.mean() < 1.0                                        # some vertices unseen, not all
    if not occlusion:
        assert (got[1] == 1).any() and (got[1] == 2).any() and (got[1] == 3).any()   # one view alone, and blends of two and three
    if occlusion:
        free = gpu_colors(s["v"], s["n"], s["imgs"], None, s["k"], s["w"], s["c"], depth_tol=0.02, fill=FILL, mode=mode)
        assert (free[1] >= got[1]).all() and (free[1] > got[1]).any()     # the depth maps do hide the far side
    again = gpu_colors(s["v"], s["n"], s["imgs"], s["depth"] if occlusion else None, s["k"], s["w"], s["c"], depth_tol=0.02, fill=FILL,
                       mode=mode)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


@pytest.mark.parametrize("n_views", [1, 64])
def test_one_view_and_the_most_views(n_views):
    assert n_views in (1, ops.MESH_MAX_VIEWS)
    got = assert_bits(sphere_scene(n_views))
    assert got[1].max() <= n_views and (got[1] > 0).any()
    if n_views == 64:
        assert got[1].max() > 16                                            # the sums do run past one upload launch's cameras


@pytest.mark.parametrize("power", [0, 8])
@pytest.mark.parametrize("mode", ["mean", "best"])
def test_weight_powers(power, mode):
    assert power in (0, ops.MESH_COLOR_MAX_POWER)
    assert_bits(sphere_scene(3), occlusion=False, power=power, mode=mode, min_cos=0.0)   # without depth maps most vertices blend 2 or 3 views


@pytest.mark.parametrize("V", [1, 63, 64, 65, BLOCK + 1])
def test_vertex_counts_round_the_wave_and_the_block(V):
    assert_bits(sphere_scene(3), V=V)


def test_no_normals_every_view_weighs_one():
    s = sphere_scene(3)
    got = gpu_colors(s["v"], None, s["imgs"], s["depth"], s["k"], s["w"], s["c"], depth_tol=0.02, fill=FILL, power=3)
    want = R.vertex_colors(s["v"], None, s["imgs"], s["depth"], s["k"], s["w"], s["c"], depth_tol=0.02, fill=FILL, power=3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------ known answers on the device
def test_affine_ramp_on_the_device():
    s = ramp_scene()
    k, w, c = cameras_of(s["K"], [s["c2w"]])
    depth = gpu_depth(s["v"], s["f"], s["K"], [s["c2w"]], s["H"], s["W"])
    normals = ops.raster_vertex_normals(cuda(s["v"]), cuda(s["f"])).cpu().numpy()
    check_ramp(*gpu_colors(s["v"], normals, s["img"], depth, k, w, c, fill=FILL), s)


def test_two_squares_on_the_device():
    s = two_squares_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    depth = gpu_depth(s["v"], s["f"], s["K"], s["c2ws"], s["H"], s["W"])
    check_two_squares(gpu_colors(s["v"], None, s["imgs"], depth, k, w, c, **s["kw"]),
                      gpu_colors(s["v"], None, s["imgs"], None, k, w, c, **s["kw"]), s)


def test_cutoffs_on_the_device():
    """the CPU test's vertices: behind the camera, one pixel out on each side, NaN and infinite ones -- and among them (3, 2, 2),
    which lands on a pixel centre (fx = fy = 0), and (6.5, 2, 2), whose x0 + 1 == W - 1"""
    s = cutoff_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    check_cutoffs(*gpu_colors(s["v"], None, s["img"], None, k, w, c, fill=FILL), s)


@pytest.mark.parametrize("power,mode,want", TWO_ANGLE_ANSWERS)
def test_power_and_mode_hand_values_on_the_device(power, mode, want):
    s = two_angle_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    colors, used = gpu_colors(s["v"], s["n"], s["imgs"], None, k, w, c, power=power, mode=mode, min_cos=0.0)
    assert used[0] == 2 and tuple(colors[0]) == (want,) * 3


def test_zero_normal_and_min_cos_on_the_device():
    s = two_angle_scene()
    k, w, c = cameras_of(s["K"], s["c2ws"])
    colors, used = gpu_colors(s["v"], np.zeros((1, 3)), s["imgs"], None, k, w, c, min_cos=0.0, fill=FILL)
    assert used[0] == 0 and tuple(colors[0]) == FILL
    colors, used = gpu_colors(s["v"], s["n"], s["imgs"], None, k, w, c, min_cos=0.8, power=0)
    assert used[0] == 2 and tuple(colors[0]) == (150,) * 3
    colors, used = gpu_colors(s["v"], s["n"], s["imgs"], None, k, w, c, min_cos=float(np.nextafter(0.8, 1.0)), power=0)
    assert used[0] == 1 and tuple(colors[0]) == (100,) * 3
    colors, _ = gpu_colors(s["v"], s["n"], s["imgs"][::-1], None, *cameras_of(s["K"], s["c2ws"][::-1]), power=0, mode="best", min_cos=0.0)
    assert tuple(colors[0]) == (200,) * 3                                  # a tie goes to the lowest view index


# ------------------------------------------------------------------ round trip through the rasteriser
RT_H, RT_W, RT_FOCAL, RT_MIN_COS, RT_SLOPE = 96, 128, 170.0, 0.5, 100.0
RT_CAMERAS, RT_HEIGHTS = 8, (2.0, -2.0)
RT_UNSEEN_CAP = 0.10


def test_round_trip_through_the_rasteriser():
    """A 2562-vertex unit icosphere is painted with colour = rint(128 + 100 * position), rendered unshaded (ambient = 1) from
    8 cameras on a ring of radius 4, heights alternating between 2 and -2, and coloured back from those renders.

    Bound on |colour - painted| for a vertex some view saw.  The field changes by 100 levels per unit length in each
    coordinate.  A texel of the vertex's footprint lies less than one pixel from its projection in x and in y; a pixel spans
    z / f of length across the ray at depth z <= |eye| + 1, and 1 / cos as much along a surface seen at cos.  The vertex passed
    cos >= 0.5; the faces under its footprint are its own and their neighbours, whose normals turn by at most delta = the
    longest edge over the radius, so cos_eff = cos(arccos(0.5) + delta).  Hence the surface point under a texel lies within
    dp = sqrt(2) * ((|eye| + 1) / f) / cos_eff of the vertex, and the field there within 100 * dp of the field at the vertex.  Four
    roundings of at most half a level each come on top: the painted vertex colours, the rendered pixel, the colour written
    here, and the painted colour it is compared with.  The blend over texels and over views is a convex combination, which
    adds nothing.  bound = 100 * dp + 2, about 13 levels of the 200 the field spans.

    Cap on the unseen share: 0.10.  The restatement on the CPU, with depth maps from raster_ref, leaves 21.9 % of this sphere
    unseen from 6 cameras at heights +-1.5 (562 of 2562: towards the poles every camera is seen at cos < 0.5), so the scene has
    8 cameras at heights +-2, from which the restatement leaves 7.3 % unseen (188 of 2562; 1732 seen once, 596 twice, 46 three
    times)."""
    v, f = R.icosphere(4)
    assert len(v) == 2562
    painted = np.rint(128.0 + RT_SLOPE * v).astype(np.uint8)
    K = R.intrinsics(RT_H, RT_W, RT_FOCAL)
    c2ws = np.stack([R.look_at((DIST * np.cos(0.1 + 2 * np.pi * i / RT_CAMERAS), DIST * np.sin(0.1 + 2 * np.pi * i / RT_CAMERAS),
                                RT_HEIGHTS[i % 2])) for i in range(RT_CAMERAS)])
    cams = [(K.astype(np.float32), np.linalg.inv(c).astype(np.float32)) for c in c2ws]
    tv, tf = cuda(v), cuda(f)
    renders = []
    for Kc, E in cams:
        k_inv, c32 = CM.ray_camera(Kc, E)
        renders.append(ops.raster_frames(tv, tf, k_inv, c32[None], RT_H, RT_W, colors=cuda(painted), ambient=1.0)["image"][0].cpu().numpy())
    colors, used, state = CMesh.color_mesh(v, f, cams, renders, min_cos=RT_MIN_COS, fill_rounds=0)
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).max()
    cos_eff = np.cos(np.arccos(RT_MIN_COS) + edge / 1.0)
    bound = RT_SLOPE * np.sqrt(2.0) * ((np.linalg.norm(c2ws[:, :3, 3], axis=1).max() + 1.0) / RT_FOCAL) / cos_eff + 2.0
    seen = used > 0
    err = np.abs(colors[seen].astype(np.int32) - painted[seen].astype(np.int32)).max()
    print(f"bound {bound:.2f}, worst error {err}, unseen share {(~seen).mean():.4f} (cap {RT_UNSEEN_CAP})")
    assert err <= bound
    assert (~seen).mean() <= RT_UNSEEN_CAP
    assert np.array_equal(state == CMesh.STATE_SEEN, seen) and (state[~seen] == CMesh.STATE_EMPTY).all()


# ------------------------------------------------------------------ fill
def cap_scene():
    v, f = R.icosphere(3)
    rng = np.random.default_rng(8)
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    used = (v[:, 2] > 0.8).astype(np.uint8) * 2                      # only a cap of the sphere has colour
    colors[used == 0] = FILL
    return f, colors, used


@pytest.mark.parametrize("rounds", [0, 1, 3, 1000])
def test_fill_matches_the_restatement(rounds):
    f, colors, used = cap_scene()
    want = R.fill(f, colors, used, rounds)
    c, st, run = ops.mesh_color_fill(cuda(f), cuda(colors), cuda(used), rounds)
    c, st = c.cpu().numpy(), st.cpu().numpy()
    print(f"rounds {rounds}: run {run}, coloured {(st != 0).sum()} of {len(st)}")
    assert run == want[2] and np.array_equal(st != 0, want[1] != 0) and np.array_equal(c, want[0])
    if rounds == 0:
        assert run == 0 and np.array_equal(c, colors) and np.array_equal(st != 0, used != 0)      # the identity
    if rounds == 1000:
        assert (st != 0).all() and run < 40                                                          # finished, and stopped early
        exact = ops.mesh_color_fill(cuda(f), cuda(colors), cuda(used), run - 1)                       # without the idle round
        assert exact[2] == run - 1 and np.array_equal(exact[0].cpu().numpy(), c)                     # stopping early costs no bits


def test_fill_small_cases_on_the_device():
    f = np.array([(0, 1, 2), (0, 2, 3)], np.int32)
    colors = np.array([(0, 0, 0), (10, 1, 0), (40, 2, 1), (10, 3, 0), FILL], np.uint8)
    c, st, run = ops.mesh_color_fill(cuda(f), cuda(colors), cuda(np.array([0, 1, 1, 1, 0], np.uint8)), 5)
    assert tuple(c[0].tolist()) == (25, 2, 0) and st.tolist() == [1, 1, 1, 1, 0] and tuple(c[4].tolist()) == FILL and run == 2
    with pytest.raises(UfrError):
        ops.mesh_color_fill(cuda(np.array([(0, 1, 9)], np.int32)), cuda(colors), cuda(np.zeros(5, np.uint8)), 1)


# ------------------------------------------------------------------ argument errors
def test_argument_errors_raise_and_launch_nothing():
    import torch

    s = sphere_scene(3)
    tv, tn = cuda(s["v"]), cuda(s["n"])
    k, w, c = s["k"], s["w"], s["c"]
    imgs = cuda(s["imgs"])

    def bad(**kw):
        a = dict(verts=tv, normals=tn, images=imgs, depth=None, k=k, w2c=w, centre=c)
        a.update(kw)
        with pytest.raises(UfrError):
            ops.mesh_vertex_colors(**a)

    ops.profile_enable(True)                       # every launch of the library is recorded from here on
    bad(images=imgs[:0], k=k[:0], w2c=w[:0], centre=c[:0])                                       # no view
    many = torch.zeros((65, 4, 4, 3), dtype=torch.uint8, device="cuda")
    bad(images=many, k=np.tile(k[:1], (65, 1, 1)), w2c=np.tile(w[:1], (65, 1, 1)), centre=np.tile(c[:1], (65, 1)))
    bad(images=imgs[:, :1].contiguous())                                                           # H below 2
    bad(images=imgs[:, :, :1].contiguous())                                                        # W below 2
    bad(images=imgs.float())                                                                       # wrong dtype
    bad(images=imgs[..., :2].contiguous())                                                         # two channels
    bad(depth=torch.zeros((3, H, W + 1), dtype=torch.float32, device="cuda"))                      # depth of another size
    bad(depth=torch.zeros((3, H, W), dtype=torch.float64, device="cuda"))
    bad(power=9)
    bad(power=-1)
    bad(min_cos=1.5)
    bad(mode="median")
    bad(depth_tol=-1.0)
    bad(k=k[:2])
    ws = w.copy()
    ws[1, 2, :3] = 0.0                                                                             # a zero row: singular
    bad(w2c=ws)
    kn = k.copy()
    kn[2, 0, 2] = np.inf
    bad(k=kn)
    cn = c.copy()
    cn[0, 1] = np.nan
    bad(centre=cn)
    # the library itself refuses what ops refuses: straight through ctypes, with nothing but the cameras valid
    from uforecon_amd import _lib
    import ctypes as C

    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    fill = (C.c_uint8 * 3)(1, 2, 3)
    p = tv.data_ptr()

    def rc(n=3, h=H, wd=W, power=2, mode=0, min_cos=0.2, kk=k, ww=w, ws_bytes=1 << 16):
        return lib.ufr_color_vertices(p, None, 1, p, None, np.ascontiguousarray(kk).ctypes.data_as(dp),
                                          np.ascontiguousarray(ww).ctypes.data_as(dp), c.ctypes.data_as(dp), n, h, wd, 0.0, 0.005, min_cos,
                                          power, mode, fill, p, p, p, ws_bytes, None)

    for kw in (dict(n=0), dict(n=65), dict(h=1), dict(wd=1), dict(power=9), dict(mode=2), dict(min_cos=1.5), dict(ww=ws), dict(kk=kn),
               dict(ws_bytes=8)):
        assert rc(**kw) != 0, kw
    assert b"singular" in (rc(ww=ws), lib.ufr_last_error())[1]
    assert lib.ufr_color_vertices_workspace_bytes(0) == 0 and lib.ufr_color_vertices_workspace_bytes(65) == 0
    assert lib.ufr_color_fill_round(None, 1, 1, None, None, None, None, None, None, None, None) != 0
    assert lib.ufr_color_fill_round(p, 1, 1, p, p, p, p, p, p, p, None) != 0 and b"alias" in lib.ufr_last_error()
    launched = ops.profile_read()
    ops.profile_enable(False)
    assert launched == {}, launched


# ------------------------------------------------------------------ the command
def test_command_end_to_end(tmp_path, capsys):
    root, mesh_dir, out_dir = str(tmp_path / "dtu"), str(tmp_path / "mesh"), str(tmp_path / "color")
    os.makedirs(mesh_dir)
    views, scans = [3, 11, 24], [7, 9]
    K = R.intrinsics(H, W, FOCAL)
    c2ws = R.ring_cameras(3, DIST, height=0.7)
    rng = np.random.default_rng(21)
    pics = {s: [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in views] for s in scans}
    R.write_dtu_tree(root, scans, views, K, c2ws, pics)
    meshes = {7: R.icosphere(3), 9: R.icosphere(2, radius=0.8, centre=(0.1, 0.0, 0.05))}
    for s, (v, f) in meshes.items():
        CM.write_ply(os.path.join(mesh_dir, "scan%d.ply" % s), v, f)
    assert CMesh.main(["--mesh_dir", mesh_dir, "--root_dir", root, "--out_dir", out_dir, "--scans", "7", "9", "--views", "3", "11", "24",
                       "--depth_tol", "0.02"]) == 0
    out = capsys.readouterr().out
    report = json.load(open(os.path.join(out_dir, "color_mesh.json")))
    assert sorted(report) == ["scan7", "scan9"]
    for s in scans:
        name = "scan%d" % s
        v, f, colors = dtu_eval.read_ply(os.path.join(out_dir, name + ".ply"), with_colors=True)
        v0, f0 = dtu_eval.read_ply(os.path.join(mesh_dir, name + ".ply"))
        assert np.array_equal(v, v0) and np.array_equal(f, f0) and colors.dtype == np.uint8
        cams = [CM.read_cam_file(os.path.join(root, "cameras/{:0>8}_cam.txt".format(i))) for i in views]
        want, used, state = CMesh.color_mesh(v0, f0, cams, pics[s], depth_tol=0.02)
        assert np.array_equal(colors, want)
        r = report[name]
        assert r["vertices"] == len(v0) and r["views"] == views
        assert (r["seen"], r["filled"], r["empty"]) == tuple(int((state == x).sum()) for x in (CMesh.STATE_SEEN, CMesh.STATE_FILLED,
                                                                                                CMesh.STATE_EMPTY))
        assert r["seen"] + r["filled"] + r["empty"] == r["vertices"] and r["seen"] > 0 and r["filled"] > 0
        assert r["views_used_histogram"] == np.bincount(used, minlength=4).tolist()
        assert all(k in r for k in ("normals_ms", "depth_ms", "color_ms", "fill_ms", "upload_ms"))
        assert "%s: %d vertices, %d seen" % (name, len(v0), r["seen"]) in out
        frames = RT.render_mesh(v, f, K, c2ws[:1], H, W, colors=colors)
        assert frames.shape == (1, H, W, 3) and frames.dtype == np.uint8 and len(np.unique(frames.reshape(-1, 3), axis=0)) > 10
