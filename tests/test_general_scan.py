"""The custom-scene loader (uforecon_amd/general_scan.py) on the host, the masked image planes' host form, and the
--test_general flags of the extract_geometry command.

The golden batches (tests/golden/general_scan_small.npz) went through the reference's own `GeneralFit`; what that pins and
what it does not is in tests/golden/make_golden_general_scan.py.  The comparisons and tolerances are those tests/test_dtu_scan.py
applies to `DtuScan` (tests/dtu_scan_golden.py: equality, and TOL_ULPS for the entries behind LAPACK / BLAS calls)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dtu_scan_golden as G
import general_scan_golden as S
from test_dtu_scan import SCHEMA
from uforecon_amd import _lib, extract_geometry as E, general_scan as GS, host_forms as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return S.write_scene(tmp_path_factory.mktemp("general"))


# ------------------------------------------------------------------ golden comparison
@pytest.mark.parametrize("case", ["mvimage", "blendedmvs"])
def test_host_loader_equals_the_reference_batches(scene_dir, case):
    cfg = S.cases()[case]
    scan = S.open_scan(*scene_dir, case, "cpu")
    V = cfg["n_views"]
    W, H = cfg["img_wh"]
    assert scan.metas == S.metas(case) and len(scan) == len(scan.metas) == (3 if case == "mvimage" else 5)
    batches = list(scan)
    assert len(batches) == len(scan)
    for i, batch in enumerate(batches):
        want, got = S.golden_batch(case, i), G.flat_batch(batch)
        assert set(got) == set(want) == set(SCHEMA) | {"meta"}
        assert got["meta"] == want["meta"] == "%s-%s-refview%d" % (S.golden()["root_name"], S.golden()["scan"], scan.metas[i][0])
        dims = {"V": V, "H": H, "W": W, "HW": H * W, "D": want["depth_values_org_scale"].shape[1]}
        for k, (shape, dtype) in SCHEMA.items():
            shape = tuple(dims.get(s, s) for s in shape)
            assert got[k].shape == want[k].shape == shape, (k, got[k].shape, want[k].shape)
            assert str(got[k].dtype) == str(want[k].dtype) == dtype, (k, got[k].dtype)
        G.assert_matches_golden(got, want, f"{case}/{i}")
        assert (got["start_idx"] == 0).all()
        assert np.array_equal(G.flat_batch(scan[i])["ray_d"], got["ray_d"])       # indexing = iterating


def test_quirks_of_the_reference_are_kept(scene_dir):
    scan = S.open_scan(*scene_dir, "mvimage", "cpu")
    # the kept entries are those of test_ref_view, and their sources ARE test_ref_view: the reference view repeats
    assert scan.metas == [(0, [0, 2, 3]), (2, [0, 2, 3]), (3, [0, 2, 3])]
    assert [scan.view_ids(i) for i in range(3)] == [[0, 0, 2], [2, 0, 2], [3, 0, 2]]
    g = S.golden_batch("mvimage", 0)
    assert np.array_equal(g["source_imgs"][0, 0], g["source_imgs"][0, 1]) and np.array_equal(g["ref_img"][0], g["source_imgs"][0, 0])
    # depth range: the LAST camera file read (view 2: near 426, interval 2.5), interval x 1.06
    want = np.arange(426.0, 2.5 * 1.06 * 192 + 426.0, 2.5 * 1.06, dtype=np.float32)
    assert np.array_equal(g["depth_values_org_scale"][0], want)
    # the render camera is the source camera (offset 0): ref_pose is the first source pose
    assert np.array_equal(g["ref_pose"][0], g["source_poses"][0, 0])
    # proj_matrices hold the UNSCALED world-to-camera matrices: translations in mm, not in units of the bounding sphere
    g1 = S.golden_batch("mvimage", 1)
    assert np.abs(g1["proj_matrices.stage1"][0, 1:, 0, :3, 3]).max() > 10 > np.abs(g1["w2cs"][0, :, :3, 3]).max()
    # an empty test_ref_view keeps every entry with its own sources
    every = S.open_scan(*scene_dir, "blendedmvs", "cpu")
    assert [m[0] for m in every.metas] == [0, 1, 2, 3, 4] and every.metas[0][1] == [1, 2, 3, 4] and every.view_ids(4) == [4, 3]
    # near / far of the bounding box: the first and last token of each file's depth line
    P, near, far, depth_min, interval = GS.read_cam_file(os.path.join(*scene_dir, "cams", "00000003_cam.txt"))
    assert (near, depth_min) == (429.0, 429.0) and far == pytest.approx(429.0 + 2.55 * 191) and interval == pytest.approx(2.55 * 1.06)
    assert P.dtype == np.float32 and P.shape == (4, 4)


def test_dataset_sizes_names_and_the_mask_switch(scene_dir):
    root, scan = scene_dir
    assert GS.DATASET_WH == {"blendedmvs": (768, 576), "mvimage": (960, 544)}
    assert GS.GeneralScan(root, scan, 2, [0, 1], "mvimage", False, device="cpu").img_wh == [960, 544]
    assert GS.GeneralScan(root, scan, 2, [0, 1], "blendedmvs", True, device="cpu").img_wh == [768, 576]
    # the mask applies with use_mask AND mvimage only
    kw = dict(n_views=2, test_ref_view=[1, 4], img_wh=[64, 32], device="cpu")
    plain = GS.GeneralScan(root, scan, dataset="mvimage", use_mask=False, **kw)[0]["source_imgs"]
    masked = GS.GeneralScan(root, scan, dataset="mvimage", use_mask=True, **kw)[0]["source_imgs"]
    blended = GS.GeneralScan(root, scan, dataset="blendedmvs", use_mask=True, **kw)[0]["source_imgs"]
    assert np.array_equal(plain.numpy(), blended.numpy()) and not np.array_equal(plain.numpy(), masked.numpy())
    raw = np.stack([D.imread_rgb(os.path.join(root, scan, "images", "%08d.jpg" % v)) for v in (1, 1)])
    msk = np.stack([D.imread_gray(os.path.join(root, scan, "masks", "%08d_mask.jpg" % v)) for v in (1, 1)])
    assert msk.dtype == np.uint8 and msk.shape == raw.shape[:3]
    assert np.array_equal(masked[0].numpy(), D.image_mask_planes_host(raw, msk, 32, 64))


def test_image_mask_planes_host():
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 256, (2, 60, 128, 3), dtype=np.uint8)
    masks = rng.choice(np.array([0, 254, 255], np.uint8), (2, 60, 128))
    out = D.image_mask_planes_host(imgs, masks, 32, 64, (4, 2, 4, 2))
    assert out.shape == (2, 3, 28, 56) and out.dtype == np.float32
    v = D.resize_u8(imgs, (64, 32))[:, 2:30, 4:60].astype(np.float64)
    m = D.resize_u8(masks[..., None], (64, 32))[:, 2:30, 4:60].astype(np.float64)
    assert np.array_equal(out, ((v / 255.0) * (m / 254.0)).astype(np.float32).transpose(0, 3, 1, 2))
    ones = D.image_mask_planes_host(imgs, np.full((2, 60, 128), 254, np.uint8), 30, 64)       # 254 is "all of it": the colour itself
    assert np.array_equal(ones, D.image_planes_host(imgs, 30, 64))
    assert (D.image_mask_planes_host(imgs, np.zeros((2, 60, 128), np.uint8), 30, 64) == 0).all()
    over = D.image_mask_planes_host(np.full((1, 4, 4, 3), 255, np.uint8), np.full((1, 4, 4), 255, np.uint8), 4, 4)
    assert (over == np.float32(255.0 / 254.0)).all()                                          # the reference's 254, kept
    with pytest.raises(ValueError):
        D.image_mask_planes_host(imgs, masks[:, :-1], 32, 64)


def test_grey_level_of_a_mask_file(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(6)
    grey = rng.integers(0, 256, (6, 9), dtype=np.uint8)
    Image.fromarray(grey).save(tmp_path / "grey.png")
    assert np.array_equal(D.imread_gray(tmp_path / "grey.png"), grey)                        # one channel: read as it is
    rgb = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    got = D.imread_gray(tmp_path / "rgb.png").astype(np.float64)
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    luma = (299 * r + 587 * g + 114 * b) / 1000
    assert np.abs(got - luma).max() <= 1.0                                                    # the rule of the module text, in integers


# ------------------------------------------------------------------ the one-line exits of the loader
def test_missing_pair_file_and_too_few_views(scene_dir, tmp_path, capsys):
    root, scan = scene_dir
    with pytest.raises(FileNotFoundError):
        GS.GeneralScan(str(tmp_path), "nothing", 3, [0, 1, 2], "mvimage", False, device="cpu")
    with pytest.raises(ValueError, match="3 views asked"):
        GS.GeneralScan(root, scan, 3, [0], "mvimage", False, device="cpu")
    with pytest.raises(ValueError, match="dataset"):
        GS.GeneralScan(root, scan, 3, [0, 1, 2], "dtu", False, device="cpu")
    ok = ["--out_dir", "b", "--depth_pos_encoding", "--explicit_similarity", "--mvs_depth_guide", "1", "--test_general"]
    with pytest.raises(SystemExit) as e:
        E.main(ok + ["--test_dir", str(tmp_path), "--test_scan", "nothing", "--dataset", "mvimage"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "Traceback" not in err and "pair.txt" in err.strip().splitlines()[-1]
    with pytest.raises(SystemExit) as e:
        E.main(ok + ["--test_dir", root, "--test_scan", scan, "--dataset", "mvimage", "--test_n_view", "3", "--test_ref_view", "0"])
    assert e.value.code == 2 and "--test_n_view" in capsys.readouterr().err.strip().splitlines()[-1]


# ------------------------------------------------------------------ the command's parser
def test_parser_defaults_of_the_four_flags():
    args = E.make_parser().parse_args(["--test_dir", "a", "--out_dir", "b"])
    assert args.test_general is False and args.use_mask is False and args.dataset == "blendedmvs"
    assert args.test_scan == ["5aa235f64a17b335eeaf9609", "5ba19a8a360c7c30c1c169df", "5adc6bd52430a05ecb2ffb85", "5bf7d63575c26f32dbf7413b"]
    assert args.img_wh == [800, 640] and args.original_img_wh == [1600, 1200]                 # make_parser() keeps today's defaults
    args = E.make_parser().parse_args(["--test_general", "--use_mask", "--dataset", "mvimage", "--test_scan", "a", "b"])
    assert args.test_general and args.use_mask and args.dataset == "mvimage" and args.test_scan == ["a", "b"]
    assert E.resolve_img_wh(E.parse_args([])) == ([800, 640], [1600, 1200])
    assert E.resolve_img_wh(E.parse_args(["--test_general"]))[0] == [768, 576]
    assert E.resolve_img_wh(E.parse_args(["--test_general", "--dataset", "mvimage"]))[0] == [960, 544]
    assert E.resolve_img_wh(E.parse_args(["--test_general", "--dataset", "mvimage", "--img_wh", "64", "32"]))[0] == [64, 32]
    assert E.resolve_img_wh(E.parse_args(["--img_wh", "400", "320"])) == ([400, 320], [1600, 1200])
    assert E.scan_seed("scene7") == E.scan_seed("scene7") != E.scan_seed("scene8")


# ------------------------------------------------------------------ the C surface
def test_new_symbols_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_(?:image_resize_mask_u8|view_pair_scores\w*))\s*\(([^)]*)\)\s*;", hdr):
        found[name] = (res, [p.strip() for p in params.split(",")])
    assert sorted(found) == ["ufr_image_resize_mask_u8", "ufr_view_pair_scores", "ufr_view_pair_scores_workspace_bytes"]
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}
    for name, (res, want) in found.items():
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is (C.c_int if res == "int" else C.c_size_t) and len(args) == len(want), name
        for p, a in zip(want, args):
            if "*" in p or p.startswith("ufr_stream"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is ctype[p.split()[0]], (name, p)
    from uforecon_amd.build import SOURCES
    assert "view_select.hip" in SOURCES and "frame_input.hip" in SOURCES
