"""The mesh fly-through (uforecon_amd/render_trajectory.py, csrc/raster.hip), the parts that need no GPU: the camera path against
the reference's own ``interpolate_trajectory`` (tests/golden/trajectory_slerp.npz, recorded by make_golden_trajectory.py with
scipy's Slerp and interp1d), the numpy restatement of the kernels (raster_ref.py) against hand-computed cases, the header
against the ctypes signatures, the command line's defaults and pose files, and the PLY reader's colours.

Trajectory tolerances: a restatement on float64 keys agreed with scipy 1.15.3 to 2.0e-14 on rotation entries and to 6.5e-13 on
positions of a few hundred (1e-15 relative); asserted are 1e-12 on rotation entries and 1e-12 x max|position| on positions."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import clean_mesh_ref as R
import raster_ref as RR
from test_clean_mesh import latlong_sphere
from uforecon_amd import _lib, clean_mesh as CM, dtu_eval, render_trajectory as RT, tsdf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

EXACT_K = np.array([[16, 0, 32], [0, 16, 24], [0, 0, 1]], np.float32)          # powers of two: an exact inverse
H, W = 48, 64


# ------------------------------------------------------------------ the camera path
def golden_cases():
    g = np.load(os.path.join(HERE, "golden", "trajectory_slerp.npz"))
    return g, [(str(name), int(n)) for name in g["names"] for n in g["num_views"]]


@pytest.mark.parametrize("name,n", golden_cases()[1])
def test_trajectory_equals_the_reference_function(name, n):
    g, _ = golden_cases()
    w2cs, want = g[f"{name}_w2cs"], g[f"{name}_c2ws_{n}"]
    got = RT.interpolate_trajectory(w2cs, n)
    assert got.shape == (n, 4, 4) and got.dtype == np.float64
    rot = np.abs(got[:, :3, :3] - want[:, :3, :3]).max()
    pos = np.abs(got[:, :3, 3] - want[:, :3, 3]).max()
    print(f"{name} {n}: rotation {rot:.3g}, position {pos:.3g} of {np.abs(want[:, :3, 3]).max():.3g}")
    assert rot <= 1e-12
    assert pos <= 1e-12 * np.abs(want[:, :3, 3]).max()
    assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))
    key0 = np.linalg.inv(w2cs[0])
    assert np.abs(got[0, :3, :3] - key0[:3, :3]).max() <= 1e-12 and np.array_equal(got[0, :3, 3], key0[:3, 3])
    eye = np.einsum("nij,nkj->nik", got[:, :3, :3], got[:, :3, :3])
    assert np.abs(eye - np.eye(3)).max() <= 1e-12


def test_trajectory_fixture_covers_what_it_should():
    g, cases = golden_cases()
    assert {len(g[f"{n}_w2cs"]) for n, _ in cases} == {2, 3, 5} and {n for _, n in cases} == {240, 7}
    assert np.array_equal(g["k3_loop_w2cs"][2], g["k3_loop_w2cs"][0])
    assert np.array_equal(g["k3_equal_neighbours_w2cs"][1], g["k3_equal_neighbours_w2cs"][0])
    w = g["k5_all_w2cs"]
    rel = [np.linalg.inv(w[k + 1])[:3, :3].T @ np.linalg.inv(w[k])[:3, :3] for k in range(4)]
    ang = [np.arccos(np.clip((np.trace(r) - 1) / 2, -1, 1)) for r in rel]
    assert ang[0] < 1e-4 and np.allclose(ang[1:], [0.3, 1.5, 3.0], atol=1e-9)
    with pytest.raises(ValueError):
        RT.interpolate_trajectory(w[:1])


# ------------------------------------------------------------------ the restatement against hand-computed cases
def facing_triangle(tilt_deg=0.0):
    """a triangle round (0, 0, 2) whose plane is tilted by ``tilt_deg`` about the x axis; the camera looks down +z from 0"""
    c, s = np.cos(np.radians(tilt_deg)), np.sin(np.radians(tilt_deg))
    flat = np.array([[-1.0, -1.0], [1.0, -1.0], [0.0, 1.0]])
    v = np.stack([flat[:, 0], flat[:, 1] * c, flat[:, 1] * s + 2.0], 1)
    return v, np.array([[0, 1, 2]], np.int32)


def test_restatement_on_a_triangle_facing_the_camera():
    v, f = facing_triangle()
    k_inv = R.k_inverse(EXACT_K.astype(np.float64))
    for faces in (f, f[:, ::-1]):                                           # winding does not matter
        r = RR.render(v, faces, k_inv, np.eye(4, dtype=np.float32), H, W)
        assert tuple(r["image"][24, 32]) == (255, 255, 255) and r["depth"][24, 32] == 2.0 and r["face_id"][24, 32] == 0
        assert np.allclose(r["normal"][24, 32], [0, 0, -1], atol=1e-7)      # facing the camera
        assert tuple(r["image"][0, 0]) == (255, 255, 255) and r["face_id"][0, 0] == -1 and r["depth"][0, 0] == 0
    r = RR.render(v, f, k_inv, np.eye(4, dtype=np.float32), H, W, background=(10, 20, 30), base_color=(1.0, 0.5, 0.0))
    assert tuple(r["image"][0, 0]) == (10, 20, 30) and tuple(r["image"][24, 32]) == (255, 128, 0)   # 127.5 goes to even
    assert r["close"][24, 32]                                                # ... and the restatement says so


def test_restatement_on_a_tilted_triangle():
    v, f = facing_triangle(60.0)
    k_inv = R.k_inverse(EXACT_K.astype(np.float64))
    r = RR.render(v, f, k_inv, np.eye(4, dtype=np.float32), H, W)
    want = int(np.rint(255 * (0.25 + 0.75 * 0.5)))
    assert want == 159 and tuple(r["image"][24, 32]) == (want,) * 3
    assert abs(float(r["depth"][24, 32]) - 2.0) <= 2.4e-7                   # one float32 ulp of 2
    col = np.array([[255, 0, 0], [255, 0, 0], [255, 0, 0]], np.uint8)
    r = RR.render(v, f, k_inv, np.eye(4, dtype=np.float32), H, W, colors=col, ambient=1.0)
    assert tuple(r["image"][24, 32]) == (255, 0, 0)
    n = RR.vertex_normals(v, f)                                             # one face: its own normal at every vertex
    r2 = RR.render(v, f, k_inv, np.eye(4, dtype=np.float32), H, W, normals=n)
    assert tuple(r2["image"][24, 32]) == (want,) * 3


def test_vertex_normal_restatement():
    v, f = latlong_sphere(24, 32)
    v = np.concatenate([v, [[5.0, 5.0, 5.0]]])                              # an unused vertex
    n = RR.vertex_normals(v, f)
    away = np.abs(v[:-1, 1]) < 0.9
    assert away.sum() > 400 and np.abs(np.abs(n[:-1][away]) - np.abs(v[:-1][away])).max() < 1e-2
    sign = np.sign((n[:-1][away] * v[:-1][away]).sum(1))
    assert (sign == sign[0]).all()                                           # all inward or all outward
    assert np.abs(np.linalg.norm(n[:-1], axis=1) - 1).max() < 1e-12 and np.array_equal(n[-1], [0, 0, 0])
    # a zero-area face adds zero, an out-of-range face nothing; two opposite faces cancel
    f2 = np.concatenate([f, [[0, 0, 1]], [[0, 1, len(v) + 3]]]).astype(np.int32)
    assert np.array_equal(RR.vertex_normals(v, f2), n)
    tri = np.array([[0, 1, 2], [2, 1, 0]], np.int32)                         # (small integers: the two normals cancel exactly)
    assert np.array_equal(RR.vertex_normals([[0, 0, 2], [3, 0, 2], [1, 2, 3]], tri), np.zeros((3, 3)))


def tie_image():
    """2 x 2 blocks with sums 2, 6, 10 (q.5: to the even neighbour), 3, 5 and a full block"""
    blocks = [[0, 0, 1, 1], [1, 1, 2, 2], [2, 2, 3, 3], [0, 1, 1, 1], [1, 1, 1, 2], [255, 255, 255, 255]]
    img = np.zeros((1, 2, 2 * len(blocks), 3), np.uint8)
    for i, b in enumerate(blocks):
        img[0, :, 2 * i:2 * i + 2, :] = np.array(b, np.uint8).reshape(2, 2, 1)
    return img, np.array([0, 2, 2, 1, 1, 255], np.uint8)


def test_downsample_restatement_ties_go_to_even():
    img, want = tie_image()
    out = RR.downsample(img, 2)
    assert out.shape == (1, 1, 6, 3) and all(np.array_equal(out[0, 0, :, c], want) for c in range(3))
    assert np.array_equal(RR.downsample(img, 1), img)
    three = np.full((1, 3, 3, 3), 7, np.uint8)
    three[0, 0, 0] = 12                                                      # 68 / 9 = 7.56 -> 8
    assert RR.downsample(three, 3)[0, 0, 0, 0] == 8


# ------------------------------------------------------------------ the C surface
def test_raster_signatures_match_the_header():
    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert "mesh rendering (ABI 507, additive)" in text and "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = []
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_raster_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
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
    assert sorted(found) == ["ufr_raster_downsample", "ufr_raster_frames", "ufr_raster_frames_workspace_bytes",
                             "ufr_raster_vertex_normals"]
    assert sorted(found) == sorted(n for n in _lib.SIGNATURES if n.startswith("ufr_raster_"))
    from uforecon_amd.build import SOURCES
    assert "raster.hip" in SOURCES


# ------------------------------------------------------------------ the command line
def test_parser_defaults_are_the_reference_constants():
    a = RT.make_parser().parse_args([])
    assert a.scans == [24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122]
    assert (a.views, a.num_views, a.img_wh, a.original_img_wh, a.offset_dist) == ([23, 24, 23], 240, [800, 640], [1600, 1200], 25.0)
    assert (a.supersample, a.flat, a.color, a.ambient, a.format, a.quality, a.dump_poses) == (1, False, "uniform", 0.25, "jpg", 90, None)
    a = RT.make_parser().parse_args("--views 1 2 --num_views 4 --img_wh 64 48 --supersample 2 --flat --color vertex --format png".split())
    assert (a.views, a.num_views, a.img_wh, a.supersample, a.flat, a.color, a.format) == ([1, 2], 4, [64, 48], 2, True, "vertex", "png")


def test_key_poses_intrinsics_and_pose_files_round_trip(tmp_path):
    g = np.load(os.path.join(HERE, "golden", "clean_mesh_sphere3.npz"))
    os.makedirs(tmp_path / "cameras")
    for view, i in ((23, 0), (24, 1)):
        with open(tmp_path / "cameras" / "{:0>8}_cam.txt".format(view), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join("%.9g" % x for x in row) for row in g[f"E_{i}"]) + "\n\nintrinsic\n"
                    + "\n".join(" ".join("%.9g" % x for x in row) for row in g[f"K_{i}"]) + "\n\n0 1\n")
    K0, w2cs = RT.key_poses(str(tmp_path), [23, 24, 23], offset_dist=25.0)
    assert np.array_equal(K0, g["K_0"]) and w2cs.shape == (3, 4, 4) and np.array_equal(w2cs[0], w2cs[2])
    c2w = np.linalg.inv(g["E_0"].astype(np.float64))
    c2w[:3, 3] += c2w[:3, 0] * 25.0
    assert np.allclose(np.linalg.inv(w2cs[0]), c2w, rtol=0, atol=1e-9)
    K = RT.scaled_intrinsics(K0, [800, 640], [1600, 1200])
    assert np.array_equal(K[0], g["K_0"][0].astype(np.float64) * 0.5) and np.array_equal(K[1], g["K_0"][1].astype(np.float64) * (640 / 1200))
    assert np.array_equal(K[2], g["K_0"][2])
    path = RT.interpolate_trajectory(w2cs, 4)
    j = RT.pinhole_json(K, path[1], 640, 800)
    assert j["extrinsic"][12:15] == np.linalg.inv(path[1])[:3, 3].tolist()    # column-major: the translation is entries 12..14
    assert j["intrinsic"]["intrinsic_matrix"][6:8] == [K[0, 2], K[1, 2]] and (j["intrinsic"]["width"], j["intrinsic"]["height"]) == (800, 640)
    with open(tmp_path / "tmp1.json", "w") as f:
        json.dump(j, f, indent=4)
    K2, c2w2, h2, w2 = RT.load_pinhole_json(str(tmp_path / "tmp1.json"))
    assert np.array_equal(K2, K) and (h2, w2) == (640, 800)
    assert np.abs(c2w2 - path[1]).max() <= 1e-12 * np.abs(path[1]).max()
    S = RT.supersampled_intrinsics(K, 2)
    assert np.array_equal(S[0], 2 * K[0] + 0.5 * K[2]) and np.array_equal(S[2], K[2])


def test_read_ply_with_colors(tmp_path):
    v, f = latlong_sphere(4, 5)
    col = (np.arange(len(v) * 3).reshape(-1, 3) * 7 % 256).astype(np.uint8)
    tsdf.meshwrite(str(tmp_path / "c.ply"), v, f, np.zeros_like(v), col)
    rv, rf, rc = dtu_eval.read_ply(str(tmp_path / "c.ply"), with_colors=True)
    assert np.allclose(rv, v, atol=1e-6) and np.array_equal(rf, f) and rc.dtype == np.uint8 and np.array_equal(rc, col)
    assert len(dtu_eval.read_ply(str(tmp_path / "c.ply"))) == 2                # the default is unchanged
    CM.write_ply(str(tmp_path / "m.ply"), v, f)
    rv, rf, rc = dtu_eval.read_ply(str(tmp_path / "m.ply"), with_colors=True)
    assert rc is None and np.array_equal(rf, f)
