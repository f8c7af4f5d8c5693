"""The DTU scan loader (uforecon_amd/dtu_scan.py) on the host, the restated resize and decomposition it rests on
(uforecon_amd/host_forms.py, cameras.py) and the extract_geometry command's parser.

The golden batches (tests/golden/dtu_scan_small.npz) went through the reference's own `DtuFitSparse`; what that pins and
what it does not is in tests/golden/make_golden_dtu_scan.py.  On the machine that wrote the file every key comes out equal bit
for bit.  On a second machine the entries behind LAPACK / BLAS calls moved by up to 2 float32 steps of their key's scale; those
keys are tested at four times what was measured (tests/dtu_scan_golden.py: TOL_ULPS), every other key for
equality."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import dtu_scan_golden as G
from uforecon_amd import _lib, cameras, extract_geometry as E, host_forms as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHEMA = {  # key -> (shape with V views, D hypotheses, an HxW image; dtype)
    "scale_mat": ((1, 4, 4), "float32"), "trans_mat": ((1, 4, 4), "float32"), "extrinsic_render_view": ((1, 4, 4), "float32"),
    "ref_pose": ((1, 4, 4), "float32"), "ref_pose_inv": ((1, 4, 4), "float32"),
    "w2cs": ((1, "V", 4, 4), "float32"), "source_poses": ((1, "V", 4, 4), "float32"), "source_poses_inv": ((1, "V", 4, 4), "float32"),
    "intrinsics": ((1, "V", 3, 3), "float32"), "intrinsic_render_view": ((1, 3, 3), "float32"),
    "proj_matrices.stage1": ((1, "V", 2, 4, 4), "float32"), "proj_matrices.stage2": ((1, "V", 2, 4, 4), "float32"),
    "proj_matrices.stage3": ((1, "V", 2, 4, 4), "float32"),
    "depth_values_org_scale": ((1, "D"), "float32"), "near_fars": ((1, "V", 2), "float32"),
    "ref_img": ((1, 3, "H", "W"), "float32"), "source_imgs": ((1, "V", 3, "H", "W"), "float32"), "scale_factor": ((1,), "float32"),
    "ray_o": ((1, 3), "float32"), "ray_d": ((1, 3, "HW"), "float32"), "cam_ray_d": ((1, 3, "HW"), "float32"),
    "start_idx": ((1,), "int64"),
}


@pytest.fixture(scope="module")
def scan_dir(tmp_path_factory):
    return G.write_scan(tmp_path_factory.mktemp("dtu"))


# ------------------------------------------------------------------ golden comparison
@pytest.mark.parametrize("case", ["set0", "set1"])
def test_host_loader_equals_the_reference_batches(scan_dir, case):
    cfg = G.cases()[case]
    scan = G.open_scan(*scan_dir, case, "cpu")
    V = cfg["n_views"]
    clip = cfg["clip_wh"]
    W, H = cfg["img_wh"][0] - 2 * clip[0], cfg["img_wh"][1] - 2 * clip[1]
    assert len(scan) == V
    batches = list(scan)
    assert len(batches) == V
    for i, batch in enumerate(batches):
        want, got = G.golden_batch(case, i), G.flat_batch(batch)
        assert set(got) == set(want) == set(SCHEMA) | {"meta"}
        assert got["meta"] == want["meta"] == "%s-%s-%08d" % (G.golden()["root_name"], G.golden()["scan"], i)
        n_depth = want["depth_values_org_scale"].shape[1]
        dims = {"V": V, "H": H, "W": W, "HW": H * W, "D": n_depth}
        for k, (shape, dtype) in SCHEMA.items():
            shape = tuple(dims.get(s, s) for s in shape)
            assert got[k].shape == want[k].shape == shape, (k, got[k].shape, want[k].shape)
            assert str(got[k].dtype) == str(want[k].dtype) == dtype, (k, got[k].dtype)
        G.assert_matches_golden(got, want, f"{case}/{i}")
        assert (got["start_idx"] == 0).all()
        assert np.array_equal(G.flat_batch(scan[i])["ray_d"], got["ray_d"])       # indexing = iterating


def test_quirks_of_the_reference_are_kept(scan_dir):
    g = G.golden_batch("set0", 0)
    # depth range: the LAST camera file's line (430.0 2.4 in view 33; the others say 425.0 2.5), interval x 1.06
    want = np.arange(430.0, 2.4 * 1.06 * 192 + 430.0, 2.4 * 1.06, dtype=np.float32)
    assert np.array_equal(g["depth_values_org_scale"][0], want)
    # proj_matrices: element [1, 3, 3] stays zero; stage k scales the first two intrinsic rows by 2^(k-1)
    for st, f in (("stage1", 1), ("stage2", 2), ("stage3", 4)):
        p = g["proj_matrices." + st][0]
        assert (p[:, 1, 3, 3] == 0).all() and np.array_equal(p[:, 1, :2, :3], g["intrinsics"][0][:, :2] / 4 * f)
        assert np.array_equal(p[:, 0, 3], np.tile([0, 0, 0, 1], (3, 1)))
    # ... and hold the UNSCALED world-to-camera matrices: translations in mm, not in units of the bounding sphere
    assert np.abs(g["proj_matrices.stage1"][0, 1:, 0, :3, 3]).max() > 10 > np.abs(g["w2cs"][0, :, :3, 3]).max()
    # the render camera: the source camera moved 25 mm along its own x axis
    scan = G.open_scan(*scan_dir, "set0", "cpu")
    for i in range(3):
        c2w, render = np.linalg.inv(scan.all_w2cs_original[i].numpy()), np.linalg.inv(scan.all_render_w2cs_original[i].numpy())
        assert np.allclose(render[:3, 3] - c2w[:3, 3], 25 * c2w[:3, 0], atol=1e-3) and np.allclose(render[:3, :3], c2w[:3, :3], atol=1e-6)
    # set 1 reads the fixed view list
    assert G.open_scan(*scan_dir, "set1", "cpu").idx == [43, 42]


# ------------------------------------------------------------------ the restated resize
def test_resize_constant_and_identity():
    rng = np.random.default_rng(0)
    for (Hs, Ws), (H, W) in (((60, 128), (32, 64)), ((7, 5), (3, 2)), ((33, 47), (32, 40)), ((5, 6), (11, 13)), ((60, 128), (30, 64))):
        for c in (0, 1, 127, 254, 255):
            out = D.resize_u8(np.full((Hs, Ws, 3), c, np.uint8), (W, H))
            assert out.shape == (H, W, 3) and out.dtype == np.uint8 and (out == c).all(), (Hs, Ws, H, W, c)
    img = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    assert np.array_equal(D.resize_u8(img, (14, 9)), img)


def test_resize_factor_two_in_x_alone_and_in_both():
    """Factor exactly 2 along x with the rows kept: taps 1/2, 1/2 -> row value (a + b) * 1024; the vertical weights are 2048
    and 0, so the pixel is ((2048 * ((a + b) * 64)) >> 16) + 2 >> 2 = (2 (a + b) + 2) >> 2 = (a + b + 1) >> 1: the mean of the
    two neighbours, a half rounded UP.  Factor 2 along both axes: the box mean (sum + 2) >> 2."""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (10, 16, 3), dtype=np.uint8)
    v = img.astype(np.int32)
    assert np.array_equal(D.resize_u8(img, (8, 10)), (v[:, 0::2] + v[:, 1::2] + 1) >> 1)
    box = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
    assert np.array_equal(D.resize_u8(img, (8, 5)), box)
    assert np.array_equal(D.resize_u8(np.stack([img, img[::-1]]), (8, 5))[1], D.resize_u8(img[::-1].copy(), (8, 5)))   # batched


def test_resize_edges_read_only_inside_the_image():
    """DTU's factors (2 and 1.875) and an enlargement: the taps of the last (and first) output row and column lie inside the
    source, and a tap that was moved to the edge has weight 0 along x."""
    for n_dst, n_src in ((32, 60), (64, 128), (3, 7), (2, 5), (11, 5), (13, 6)):
        for along_x in (True, False):
            s0, s1, w0, w1 = D._taps(n_dst, n_src, along_x)
            assert s0.min() >= 0 and s1.max() <= n_src - 1 and (s0 <= s1).all() and ((w0 + w1) == 2048).all()
    s0, s1, w0, w1 = D._taps(11, 5, True)
    assert s0[0] == 0 and w0[0] == 2048 and s0[-1] == 4 and w0[-1] == 2048 and w1[-1] == 0
    # the last output row of 60 -> 32: source coordinate 31.5 * 1.875 - 0.5 = 58.5625, rows 58 and 59
    s0, s1, w0, w1 = D._taps(32, 60, False)
    assert (s0[-1], s1[-1], w0[-1], w1[-1]) == (58, 59, 896, 1152)
    # an image whose last row and column are the only bright ones: they show up in the last output row / column only
    img = np.zeros((60, 128, 3), np.uint8)
    img[-1], img[:, -1] = 255, 255
    out = D.resize_u8(img, (64, 32))
    assert (out[:-1, :-1] == 0).all() and (out[-1] > 0).all() and (out[:, -1] > 0).all()


def test_image_planes_host():
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (2, 60, 128, 3), dtype=np.uint8)
    out = D.image_planes_host(imgs, 32, 64, (4, 2, 4, 2))
    assert out.shape == (2, 3, 28, 56) and out.dtype == np.float32
    small = D.resize_u8(imgs, (64, 32))[:, 2:30, 4:60]
    assert np.array_equal(out, (small.astype(np.float64) / 255.0).astype(np.float32).transpose(0, 3, 1, 2))
    with pytest.raises(ValueError):
        D.image_planes_host(imgs, 32, 64, (32, 0, 32, 0))


# ------------------------------------------------------------------ the restated decomposition
def test_decomposition_gives_back_the_camera():
    """20 seeded cameras K [R | -R c] built in float64, decomposed as float32: K, R and c come back within float32 rounding
    (K's entries are up to ~3000 and the products that make P lose a few ulps of that, hence the relative bounds)."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        R = q * np.sign(np.linalg.det(q))
        K = np.array([[rng.uniform(500, 3000), rng.uniform(-2, 2), rng.uniform(100, 900)],
                      [0, rng.uniform(500, 3000), rng.uniform(100, 700)], [0, 0, 1.0]])
        c = rng.uniform(-700, 700, 3)
        P = (K @ np.concatenate([R, (-R @ c)[:, None]], axis=1)).astype(np.float32)
        K2, R2, c2 = cameras.decompose_projection_matrix(P)
        assert K2.dtype == R2.dtype == c2.dtype == np.float32 and c2.shape == (4, 1) and c2[3, 0] == 1
        assert (np.diag(K2) > 0).all() and np.allclose(np.tril(K2, -1), 0, atol=1e-3)
        assert np.allclose(K2, K, rtol=2e-6, atol=2e-3)
        assert np.allclose(R2, R, atol=2e-6)
        assert np.allclose(c2[:3, 0], c, rtol=1e-5, atol=2e-3)
        intr, pose = cameras.load_K_Rt_from_P(P)
        assert intr.dtype == np.float64 and pose.dtype == np.float32 and np.allclose(pose[:3, :3], R.T, atol=2e-6)


# ------------------------------------------------------------------ the command's parser
def test_parser_has_the_reference_flags_and_defaults():
    ref = {f["flag"]: f for f in json.loads(str(G.golden()["main_py_flags"]))}
    parser = E.make_parser()
    ours = {a.option_strings[0]: a for a in parser._actions if a.option_strings and a.option_strings[0] != "-h"}
    own = {"--scans", "--img_wh", "--original_img_wh", "--seed", "--precision"}
    wanted = {"--test_dir", "--out_dir", "--load_ckpt", "--test_n_view", "--test_ref_view", "--set", "--test_sample_coarse",
              "--test_sample_fine", "--test_coarse_only", "--test_ray_num", "--mvs_depth_guide", "--depth_pos_encoding",
              "--explicit_similarity", "--use_dir_srdf", "--ndepths", "--depth_inter_r", "--cr_base_chs", "--volume_type"}
    assert wanted <= set(ours) and own <= set(ours) and wanted <= set(ref) and not (own & set(ref))
    for flag, a in ours.items():
        if flag in own:
            continue
        r = ref[flag]                                    # every other flag is one of main.py's
        if r["action"] == "store_true":
            assert a.nargs == 0 and a.default is False and a.const is True, flag
        else:
            assert a.default == r["default"] and a.nargs == r["nargs"], (flag, a.default, r["default"])
            assert getattr(a.type, "__name__", None) == r["type"] and (a.choices or None) == r["choices"], flag
    args = parser.parse_args(["--test_dir", "a", "--out_dir", "b"])
    assert args.test_n_view == 3 and args.set == 0 and args.scans == [24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122]
    assert args.img_wh == [800, 640] and args.original_img_wh == [1600, 1200] and args.seed == 0


@pytest.mark.parametrize("extra", [["--volume_type", "featuregrid"], ["--volume_type", "tsdf"], ["--use_dir_srdf"],
                                   ["--ndepths", "64,32,8"], ["--mvs_depth_guide", "0"], ["--test_n_view", "8"]])
def test_unimplemented_flag_values_exit_with_one_line(extra, capsys):
    ok = ["--test_dir", "a", "--out_dir", "b", "--depth_pos_encoding", "--explicit_similarity", "--mvs_depth_guide", "1"]
    assert E.unimplemented(E.make_parser().parse_args(ok)) is None
    with pytest.raises(SystemExit) as e:
        E.main(ok + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "Traceback" not in err and extra[0] in err.strip().splitlines()[-1]


def test_view_uniforms_depend_on_seed_scan_and_view_only():
    a = E.view_uniforms(0, 24, 1, 4, 3, 10)
    b = E.view_uniforms(0, 24, 1, 4, 3, 10)
    assert a[0].shape == (4, 10) and a[1].shape == (3, 10) and all((x == y).all() for x, y in zip(a, b))
    for other in ((1, 24, 1), (0, 37, 1), (0, 24, 2)):
        assert not (E.view_uniforms(*other, 4, 3, 10)[0] == a[0]).all()
    assert E.view_uniforms(0, 24, 1, 4, 3, 10, coarse_only=True)[1] is None


# ------------------------------------------------------------------ the C surface
def test_new_symbols_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_(?:image_resize_u8|pixel_rays))\s*\(([^)]*)\)\s*;", hdr):
        found[name] = [p.strip() for p in params.split(",")]
    assert sorted(found) == ["ufr_image_resize_u8", "ufr_pixel_rays"]
    for name, want in found.items():
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is C.c_int and len(args) == len(want), name
        for p, a in zip(want, args):
            if "*" in p or p.startswith("ufr_stream"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is C.c_int32 and p.split()[0] == "int32_t", (name, p)
    from uforecon_amd.build import SOURCES
    assert "frame_input.hip" in SOURCES
