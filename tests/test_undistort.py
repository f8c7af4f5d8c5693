"""Undistortion on the host (uforecon_amd/undistort.py): the numpy host form of ufr_image_undistort_u8 against the per-pixel
statement of the header's rule (tests/undistort_ref.py), the geometry of the resampled picture, the zoom, the converter's
``--undistort`` on a synthetic COLMAP model, and the C surface."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import undistort_ref as R
from uforecon_amd import _lib, colmap2mvsnet as C, undistort as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLYNOMIAL4 = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
FISHEYE3 = ("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")


def small_source(C_, n=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 7, 9, C_), dtype=np.uint8)


def ref_arrays(src, model, params, k_out, H, W):
    dst, valid, _, _ = R.undistort(src.tolist(), model, params, k_out, H, W)
    return np.array(dst, np.uint8).reshape(len(src), H, W, src.shape[3]), np.array(valid, np.uint8).reshape(H, W)


# ------------------------------------------------------------------ host form == the header's rule
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("model", POLYNOMIAL4 + ("SIMPLE_PINHOLE", "PINHOLE"))
def test_host_form_equals_the_rule_polynomial(model, channels):
    src, params = small_source(channels), R.SMALL_CAMERAS[model]
    got = U.undistort_host(src, model, params, R.K_SMALL, 6, 8)
    if model in POLYNOMIAL4:
        assert 0 < int((got[1] == 0).sum()) < 48            # strong enough: some output pixels have no source, some have one
    R.assert_same(got, ref_arrays(src, model, params, R.K_SMALL, 6, 8))
    assert not got[0][:, got[1] == 0].any() and set(np.unique(got[1])) <= {0, 255}


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("model", FISHEYE3)
def test_host_form_equals_the_rule_fisheye(model, channels):
    """atan may differ in the last place between numpy and `math`: one level is allowed at a value within 1e-9 of a half-integer
    and a `valid` flip at a position within 1e-9 of a bound -- and these inputs hold no such pixel, so nothing differs here."""
    src, params = small_source(channels), R.SMALL_CAMERAS[model]
    got = U.undistort_host(src, model, params, R.K_SMALL, 6, 8)
    assert 0 < int((got[1] == 0).sum()) < 48
    ys, xs = np.meshgrid(np.arange(6), np.arange(8), indexing="ij")
    u, v, _ = U.source_map_host(model, params, R.K_SMALL, 7, 9, xs, ys)
    val = U.undistort_host(src, model, params, R.K_SMALL, 6, 8, unrounded=True)[0]
    ties = R.tie_pixels(val, u, v, 7, 9)
    assert not (ties[0] & (got[1] == 255)[None, :, :, None]).any() and not ties[1].any()
    R.assert_same(got, ref_arrays(src, model, params, R.K_SMALL, 6, 8), ties)


def test_the_map_and_the_distortion_equal_the_rule():
    for model, params in R.SMALL_CAMERAS.items():
        xs, ys = np.array([0, 3, 7, 2]), np.array([0, 2, 5, 4])
        u, v, valid = U.source_map_host(model, params, R.K_SMALL, 7, 9, xs, ys)
        for k in range(4):
            ru, rv = R.source_of(model, params, R.K_SMALL, int(xs[k]), int(ys[k]))
            assert math.isclose(u[k], ru, rel_tol=0, abs_tol=1e-12) and math.isclose(v[k], rv, rel_tol=0, abs_tol=1e-12), (model, k)
            assert bool(valid[k]) == (0 <= ru <= 8 and 0 <= rv <= 6)
        xd, yd = U.distort_host(model, params, np.array([0.3, 0.0]), np.array([-0.2, 0.0]))
        rx, ry = R.distort(model, params, 0.3, -0.2)
        assert math.isclose(xd[0], rx, abs_tol=1e-15) and math.isclose(yd[0], ry, abs_tol=1e-15) and xd[1] == 0 and yd[1] == 0


@pytest.mark.parametrize("model", ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV"])
def test_zero_distortion_with_dyadic_intrinsics_is_the_identity(model):
    """f = 64, c = (32.5, 24.5): every operation of the rule is exact, u = x and v = y"""
    n_params, single = C.CAMERA_MODELS[C.MODEL_IDS[model]][1:]
    params = np.zeros(n_params)
    params[:3 if single else 4] = (64.0, 32.5, 24.5) if single else (64.0, 64.0, 32.5, 24.5)
    src = np.random.default_rng(3).integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    dst, valid = U.undistort_host(src, model, params, (64.0, 64.0, 32.5, 24.5), 48, 64)
    assert np.array_equal(dst, src) and (valid == 255).all()


# ------------------------------------------------------------------ geometry
GEOMETRY = {"simple_radial_barrel": ("SIMPLE_RADIAL", (110.0, 63.2, 47.6, -0.25)),
            "simple_radial_pincushion": ("SIMPLE_RADIAL", (110.0, 63.2, 47.6, 0.2)),
            "radial": ("RADIAL", (110.0, 63.2, 47.6, -0.3, 0.12)),
            "opencv": ("OPENCV", (110.0, 108.0, 63.2, 47.6, -0.28, 0.09, 0.004, -0.003)),
            "full_opencv": ("FULL_OPENCV", (110.0, 108.0, 63.2, 47.6, -0.28, 0.09, 0.004, -0.003, 0.01, 0.02, -0.01, 0.005)),
            "opencv_fisheye": ("OPENCV_FISHEYE", (110.0, 108.0, 63.2, 47.6, -0.02, 0.01, -0.003, 0.001))}
GEOMETRY_BOUND = 1.25        # 0.5 source rounding + 0.5 output rounding + bilinear (1/8) 2 100 (2 pi / 64)^2 = 0.241


def wave(u, v):
    return 127.5 + 100.0 * math.sin(2 * math.pi * u / 64) * math.cos(2 * math.pi * v / 64)


@pytest.fixture(scope="module")
def wave_picture():
    return np.array([[[round(wave(x + 0.5, y + 0.5))] for x in range(128)] for y in range(96)], np.uint8)[None]


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_every_valid_pixel_shows_the_scene_at_its_own_source_position(case, wave_picture):
    model, params = GEOMETRY[case]
    p = R.named(model, params)
    k_out = (p["fx"], p["fy"], p["cx"], p["cy"])                  # the output camera keeps the focal lengths
    dst, valid = U.undistort_host(wave_picture, model, params, k_out, 96, 128)
    worst, n_valid = 0.0, 0
    for y in range(96):
        for x in range(128):
            u, v = R.source_of(model, params, k_out, x, y)
            inside = 0 <= u <= 127 and 0 <= v <= 95
            assert inside == (valid[y, x] == 255), (x, y, u, v)
            if inside:
                worst, n_valid = max(worst, abs(float(dst[0, y, x, 0]) - wave(u + 0.5, v + 0.5))), n_valid + 1
    print(f"{case}: worst {worst:.4f} levels over {n_valid} valid pixels")
    assert n_valid > 96 * 128 // 2 and worst <= GEOMETRY_BOUND


# ------------------------------------------------------------------ the zoom
def test_fit_zoom():
    K = np.array([[110.0, 0, 63.2], [0, 110.0, 47.6], [0, 0, 1]])
    src = np.zeros((1, 96, 128, 1), np.uint8)
    all_valid = lambda params, z: bool((U.undistort_host(src, "SIMPLE_RADIAL", params, U.zoomed(K, z), 96, 128)[1] == 255).all())  # noqa: E731
    barrel, pincushion = (110.0, 63.2, 47.6, -0.25), (110.0, 63.2, 47.6, 0.2)
    assert U.fit_zoom("SIMPLE_RADIAL", barrel, K, 96, 128) == 1.0 and all_valid(barrel, 1.0)
    z = U.fit_zoom("SIMPLE_RADIAL", pincushion, K, 96, 128)
    share = float((U.undistort_host(src, "SIMPLE_RADIAL", pincushion, K, 96, 128)[1] == 255).mean())
    print(f"zoom {z:.6f}; valid share at zoom 1: {share:.4f}")
    assert 1.0 < z < U.ZOOM_MAX and all_valid(pincushion, z) and not all_valid(pincushion, z - 1e-6)
    assert not all_valid(pincushion, 1.0) and 0.5 < share < 1.0                 # "keep" leaves blank pixels
    with pytest.raises(ValueError, match="blank"):
        U.fit_zoom("SIMPLE_RADIAL", (110.0, 63.2, 47.6, 5000.0), K, 96, 128)
    for model in ("FOV", "THIN_PRISM_FISHEYE", 7, 10, 11):
        with pytest.raises(ValueError, match="cannot be undistorted"):
            U.model_name(model)


# ------------------------------------------------------------------ the converter
def synthetic_scene(root, model="SIMPLE_RADIAL", params=(55.0, 31.6, 23.8, 0.2)):
    """3 pictures of 64 x 48 by one camera, 40 points that every image observes; a mask for the first picture only"""
    from PIL import Image

    rng = np.random.default_rng(11)
    dense = str(root)
    cameras = {1: C.Camera(1, model, 64, 48, np.array(params, np.float64))}
    pts = rng.uniform(-1, 1, (40, 3)) + [0, 0, 5]
    images, points = {}, {}
    for k in (1, 2, 3):
        angle = 0.1 * (k - 2)
        q = np.array([math.cos(angle / 2), 0.0, math.sin(angle / 2), 0.0])
        images[k] = C.Image(k, q, np.array([0.3 * (k - 2), 0.0, 0.0]), 1, "view %d.png" % k, rng.uniform(0, 48, (40, 2)), np.arange(40, dtype=np.int64))
    for p in range(40):
        points[p] = C.Point3D(p, pts[p], np.array([9, 9, 9]), 0.5, np.array([1, 2, 3], np.int32), np.full(3, p, np.int32))
    C.write_model(os.path.join(dense, "sparse", "0"), cameras, images, points)
    os.makedirs(os.path.join(dense, "images"))
    os.makedirs(os.path.join(dense, "masks"))
    ys, xs = np.meshgrid(np.arange(48), np.arange(64), indexing="ij")
    for k in (1, 2, 3):
        rgb = np.stack([127 + 100 * np.sin(xs / (5.0 + k)) * np.cos(ys / 7.0), 2.0 * xs + k, 3.0 * ys + 5 * k], axis=-1)
        Image.fromarray(rgb.astype(np.uint8), "RGB").save(os.path.join(dense, "images", "view %d.png" % k))
    disc = (((xs - 30) ** 2 + (ys - 22) ** 2) < 18 ** 2).astype(np.uint8) * 255
    Image.fromarray(disc, "L").save(os.path.join(dense, "masks", "view 1.png.png"))
    return dense


def files_of(dense):
    return {os.path.relpath(os.path.join(d, f), dense): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(dense) for f in fs}


def test_converter_undistorts_a_synthetic_model(tmp_path):
    from PIL import Image

    plain_dir, flag_dir = synthetic_scene(tmp_path / "plain"), synthetic_scene(tmp_path / "flag")
    sources = files_of(plain_dir)
    plain = C.convert(plain_dir, device="cpu")
    out = C.convert(flag_dir, device="cpu", undistort=True)
    cameras, images, _ = C.read_model(os.path.join(flag_dir, "sparse", "0"))
    # without the flag: what the converter wrote before the flag existed -- K as read, the pictures and the one mask copied
    after = files_of(plain_dir)
    assert set(after) - set(sources) == {"pair.txt", "cams/pair.txt", "masks/00000000_mask.jpg"} | {
        "cams/%08d_cam.txt" % i for i in range(3)} | {"images/%08d.jpg" % i for i in range(3)}
    assert all(after[k] == sources[k] for k in sources)
    for i in range(3):
        assert after["images/%08d.jpg" % i] == sources["images/view %d.png" % (i + 1)]
        assert np.array_equal(plain["intrinsics"][i], C.intrinsic_of(cameras[1])) and plain["zoom"][i] == 1.0
        assert after["cams/%08d_cam.txt" % i].decode() == C.cam_text(plain["extrinsics"][i], C.intrinsic_of(cameras[1]), plain["depth_ranges"][i])
    assert after["masks/00000000_mask.jpg"] == sources["masks/view 1.png.png"] and plain["distorted_models"] == ["SIMPLE_RADIAL"]
    # with it: K' = K with z f, in the dict, the camera files and the depth line
    z = U.fit_zoom("SIMPLE_RADIAL", cameras[1].params, C.intrinsic_of(cameras[1]), 48, 64)
    assert 1.0 < z < 1.5 and (out["zoom"] == z).all() and np.array_equal(out["intrinsics_source"], plain["intrinsics"])
    offsets, obs, points = C.observation_lists(images, C.read_model(os.path.join(flag_dir, "sparse", "0"))[2])
    for i in range(3):
        Kz = out["intrinsics"][i]
        assert Kz[0, 0] == z * 55.0 and Kz[1, 1] == z * 55.0 and Kz[0, 2] == 31.6 and Kz[1, 2] == 23.8
        text = open(os.path.join(flag_dir, "cams", "%08d_cam.txt" % i)).read()
        lines = text.splitlines()
        assert np.array_equal(np.array(" ".join(lines[7:10]).split(), np.float64).reshape(3, 3), Kz)
        want = C.depth_range(Kz, out["extrinsics"][i], points[obs[offsets[i]:offsets[i + 1]]], 0, 1)
        assert lines[11] == "%f %f %f %f" % tuple(want) and text == out["cam_texts"][i]
        assert want[2] != plain["depth_ranges"][i][2]                       # depth_num follows K'
    assert out["pair_text"] == plain["pair_text"] and np.array_equal(out["score"], plain["score"])
    for rel in ("pair.txt", "cams/pair.txt"):
        assert open(os.path.join(flag_dir, rel)).read() == open(os.path.join(plain_dir, rel)).read()
    # pictures and masks: written for every image, JPEG, the source size; "inside" leaves no blank pixel
    memory = C.convert(flag_dir, device="cpu", undistort=True, write=False)
    cam = cameras[1]
    for i in range(3):
        with Image.open(os.path.join(flag_dir, "images", "%08d.jpg" % i)) as im:
            assert im.format == "JPEG" and im.mode == "RGB" and im.size == (64, 48)
            assert np.abs(np.array(im, np.int64) - memory["images"][i]).mean() < 3       # quality 95, 4:4:4: about a level
        with Image.open(os.path.join(flag_dir, "masks", "%08d_mask.jpg" % i)) as im:
            assert im.format == "JPEG" and im.mode == "L" and im.size == (64, 48)
            assert np.abs(np.array(im, np.int64) - memory["masks"][i]).mean() < 3
        assert (memory["valid"][i] == 255).all()
        src = np.array(Image.open(os.path.join(flag_dir, "images", "view %d.png" % (i + 1))).convert("RGB"))
        assert np.array_equal(memory["images"][i], U.undistort_host(src[None], cam.model, cam.params, out["intrinsics"][i], 48, 64)[0][0])
    disc = np.array(Image.open(os.path.join(flag_dir, "masks", "view 1.png.png")))
    assert np.array_equal(memory["masks"][0], U.undistort_host(disc[None, :, :, None], cam.model, cam.params, out["intrinsics"][0], 48, 64)[0][0, :, :, 0])
    assert 0 < (memory["masks"][0] > 127).mean() < 1 and (memory["masks"][1] == 255).all() and (memory["masks"][2] == 255).all()
    # "keep": the focal length stays, blank pixels stay, and the masks are 0 there
    keep = C.convert(flag_dir, device="cpu", undistort=True, undistort_fit="keep", write=False)
    assert (keep["zoom"] == 1.0).all() and np.array_equal(keep["intrinsics"], plain["intrinsics"])
    blank = keep["valid"][1] == 0
    assert 0 < blank.mean() < 0.5 and not keep["masks"][1][blank].any() and (keep["masks"][1][~blank] == 255).all()
    assert not keep["images"][1][blank].any() and not keep["masks"][0][blank].any()


def test_pinhole_cameras_are_copied_under_the_flag(tmp_path):
    dense = synthetic_scene(tmp_path / "pinhole", "SIMPLE_PINHOLE", (55.0, 31.6, 23.8))
    sources = files_of(dense)
    out = C.convert(dense, device="cpu", undistort=True)
    after = files_of(dense)
    assert (out["zoom"] == 1.0).all() and out["distorted_models"] == [] and "masks/00000001_mask.jpg" not in after
    assert all(after["images/%08d.jpg" % i] == sources["images/view %d.png" % (i + 1)] for i in range(3))


def test_unsupported_models_and_fits_end_the_command_with_one_line(tmp_path, capsys):
    def last_line(argv):
        with pytest.raises(SystemExit) as e:
            C.main(argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "Traceback" not in err
        return err.strip().splitlines()[-1]

    fov = synthetic_scene(tmp_path / "fov", "FOV", (55.0, 55.0, 31.6, 23.8, 0.9))
    line = last_line(["--dense_folder", fov, "--undistort", "--test"])
    assert "FOV" in line and "camera 1" in line
    prism = synthetic_scene(tmp_path / "prism", "THIN_PRISM_FISHEYE", (55.0, 55.0, 31.6, 23.8) + (0.0,) * 8)
    assert "THIN_PRISM_FISHEYE" in last_line(["--dense_folder", prism, "--undistort", "--test"])
    radial = synthetic_scene(tmp_path / "radial")
    assert "--undistort_fit" in last_line(["--dense_folder", radial, "--undistort", "--undistort_fit", "outside", "--test"])
    with pytest.raises(C.ColmapError, match="undistort_fit"):
        C.convert(radial, device="cpu", undistort=True, undistort_fit="outside", write=False)
    hopeless = synthetic_scene(tmp_path / "hopeless", "SIMPLE_RADIAL", (55.0, 31.6, 23.8, 5000.0))
    assert "camera 1" in last_line(["--dense_folder", hopeless, "--undistort", "--test"])
    assert not os.path.exists(os.path.join(radial, "cams"))
    flags = {a.option_strings[0]: a.default for a in C.make_command_parser()._actions}
    assert flags["--undistort"] is False and flags["--undistort_fit"] == "inside"


# ------------------------------------------------------------------ the C surface
def test_new_symbol_in_header_binding_and_sources():
    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.findall(r"\bint\s+(ufr_image_undistort\w*)\s*\(([^)]*)\)\s*;", hdr)
    assert [name for name, _ in found] == ["ufr_image_undistort_u8"]
    want = [p.strip() for p in found[0][1].split(",")]
    rtype, args = _lib.SIGNATURES["ufr_image_undistort_u8"]
    assert rtype is ctypes.c_int and len(args) == len(want) == 13
    for p, a in zip(want, args):
        if p.startswith("const double*"):
            assert a is ctypes.POINTER(ctypes.c_double), p
        elif "*" in p or p.startswith("ufr_stream"):
            assert a is ctypes.c_void_p, p
        else:
            assert p.split()[0] == "int32_t" and a is ctypes.c_int32, p
    from uforecon_amd.build import SOURCES
    assert "undistort.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "uforecon_amd", "csrc", "undistort.hip"))
    # the models the header, the kernel's table and the host form accept are COLMAP's ids
    assert {C.MODEL_IDS[m] for m in U.SUPPORTED_MODELS} == {i for i, _ in R.MODELS.values()} == {0, 1, 2, 3, 4, 5, 6, 8, 9}
    assert all(len(names) == C.CAMERA_MODELS[i][1] for i, names in R.MODELS.values())
