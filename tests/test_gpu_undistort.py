"""The undistortion kernel (csrc/undistort.hip, ufr_image_undistort_u8) against its host form (uforecon_amd/undistort.py, which
tests/test_undistort.py holds against the header's rule), its argument errors, and the converter's ``--undistort`` on the device
against the host run."""
import ctypes as C

import numpy as np
import pytest
import torch

import undistort_ref as R
from test_undistort import FISHEYE3, synthetic_scene
from uforecon_amd import _lib, colmap2mvsnet as M, ops, undistort as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1


def check_kernel(src, model, params, k_out, H, W):
    """bytes and valid equal the host form's; for a fisheye model with the tie rule of tests/test_undistort.py (the device's
    atan may differ from numpy's in the last place)"""
    Hs, Ws = src.shape[1:3]
    dst, valid = ops.image_undistort_u8(torch.from_numpy(src).to(DEV), model, params, k_out, H, W)
    assert tuple(dst.shape) == (len(src), H, W, src.shape[3]) and tuple(valid.shape) == (H, W)
    want = U.undistort_host(src, model, params, k_out, H, W)
    ties = None
    if model in FISHEYE3:
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        u, v, _ = U.source_map_host(model, params, k_out, Hs, Ws, xs, ys)
        ties = R.tie_pixels(U.undistort_host(src, model, params, k_out, H, W, unrounded=True)[0], u, v, Hs, Ws)
    R.assert_same((dst.cpu().numpy(), valid.cpu().numpy()), want, ties)
    return want


def source(n, Hs, Ws, channels, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, Hs, Ws, channels), dtype=np.uint8)


@pytest.mark.parametrize("n,channels", [(1, 1), (3, 3), (3, 4), (1, 2)])
@pytest.mark.parametrize("model", sorted(R.SMALL_CAMERAS))
def test_kernel_equals_host_form(model, n, channels):
    want = check_kernel(source(n, 7, 9, channels), model, R.SMALL_CAMERAS[model], R.K_SMALL, 6, 8)
    assert (want[1] == 255).any()


@pytest.mark.parametrize("model", ["OPENCV", "FULL_OPENCV", "OPENCV_FISHEYE"])
def test_kernel_equals_host_form_past_one_block(model):
    """67 x 5 = 335 output pixels: rows wider than a wave, more than one 256-thread block, the last one partly empty"""
    k_out = (40.0, 4.0, 33.3, 2.6)
    want = check_kernel(source(3, 7, 9, 3, seed=1), model, R.SMALL_CAMERAS[model], k_out, 5, 67)
    assert 0 < (want[1] == 255).sum() < 335


def test_one_pixel_every_pixel_invalid_and_a_null_valid():
    params = R.SMALL_CAMERAS["RADIAL"]
    want = check_kernel(source(2, 7, 9, 3), "RADIAL", params, (6.0, 6.0, 0.5, 0.5), 1, 1)              # 1 x 1, looking at the centre
    assert want[1][0, 0] == 255
    check_kernel(source(1, 1, 1, 1), "SIMPLE_PINHOLE", (1.0, 0.5, 0.5), (1.0, 1.0, 0.5, 0.5), 1, 1)      # a 1 x 1 source too
    want = check_kernel(source(2, 7, 9, 3), "RADIAL", params, (6.0, 6.0, -400.0, 3.0), 6, 8)            # looking past the picture
    assert not want[1].any() and not want[0].any()
    src = source(3, 7, 9, 3)
    dst, valid = ops.image_undistort_u8(torch.from_numpy(src).to(DEV), "OPENCV", R.SMALL_CAMERAS["OPENCV"], R.K_SMALL, 6, 8, want_valid=False)
    assert valid is None and np.array_equal(dst.cpu().numpy(), U.undistort_host(src, "OPENCV", R.SMALL_CAMERAS["OPENCV"], R.K_SMALL, 6, 8)[0])


def test_argument_errors_and_the_next_valid_call():
    lib = _lib.load()
    src_host = source(1, 7, 9, 3)
    src = torch.from_numpy(src_host).to(DEV)
    dst = torch.zeros(1, 6, 8, 3, dtype=torch.uint8, device=DEV)
    valid = torch.zeros(6, 8, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    doubles = lambda v: (C.c_double * len(v))(*v)  # noqa: E731
    good = dict(src=src.data_ptr(), n=1, Hs=7, Ws=9, C=3, model=4, params=doubles(R.SMALL_CAMERAS["OPENCV"]), k_out=doubles(R.K_SMALL),
                H=6, W=8, dst=dst.data_ptr(), valid=valid.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.ufr_image_undistort_u8(a["src"], a["n"], a["Hs"], a["Ws"], a["C"], a["model"], a["params"], a["k_out"], a["H"], a["W"],
                                          a["dst"], a["valid"], stream)

    nan_params = list(R.SMALL_CAMERAS["OPENCV"])
    nan_params[5] = float("nan")
    bad = [dict(src=None), dict(dst=None), dict(params=None), dict(k_out=None), dict(n=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=-1),
           dict(C=0), dict(C=5), dict(model=7), dict(model=10), dict(model=11), dict(model=-1), dict(params=doubles(nan_params)),
           dict(k_out=doubles((5.5, float("inf"), 4.1, 3.2))), dict(k_out=doubles((5.5, 5.25, float("nan"), 3.2))),
           dict(k_out=doubles((0.0, 5.25, 4.1, 3.2))), dict(k_out=doubles((5.5, -1.0, 4.1, 3.2))),
           dict(Hs=65536, Ws=32768), dict(H=32768, W=65536)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
        assert b"ufr_image_undistort_u8" in lib.ufr_last_error(), (kw, lib.ufr_last_error())
    torch.cuda.synchronize()
    assert not dst.any() and not valid.any()                                   # nothing was launched
    assert call() == 0
    want = U.undistort_host(src_host, "OPENCV", R.SMALL_CAMERAS["OPENCV"], R.K_SMALL, 6, 8)
    assert np.array_equal(dst.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), want[1])
    with pytest.raises(ops.UfrError):
        ops.image_undistort_u8(src, "OPENCV", R.SMALL_CAMERAS["RADIAL"], R.K_SMALL, 6, 8)     # RADIAL's parameter count
    with pytest.raises(ops.UfrError):
        ops.image_undistort_u8(src, "FOV", (6.0, 6.0, 4.4, 3.6, 0.9), R.K_SMALL, 6, 8)
    with pytest.raises(ops.UfrError):
        ops.image_undistort_u8(src.cpu(), "OPENCV", R.SMALL_CAMERAS["OPENCV"], R.K_SMALL, 6, 8)


def test_command_names_the_model_without_the_flag_and_writes_with_it(tmp_path, capsys):
    import os

    dense = synthetic_scene(tmp_path / "scene")
    assert M.main(["--dense_folder", dense]) == 0
    note = [line for line in capsys.readouterr().err.splitlines() if "SIMPLE_RADIAL" in line]
    assert len(note) == 1 and "--undistort" in note[0]
    plain = open(os.path.join(dense, "cams", "00000001_cam.txt")).read()
    assert M.main(["--dense_folder", dense, "--undistort"]) == 0
    assert "SIMPLE_RADIAL" not in capsys.readouterr().err
    host = M.convert(dense, device="cpu", undistort=True, write=False)
    assert open(os.path.join(dense, "cams", "00000001_cam.txt")).read() == host["cam_texts"][1] != plain
    assert all(os.path.exists(os.path.join(dense, "masks", "%08d_mask.jpg" % i)) for i in range(3))


@pytest.mark.parametrize("fit", ["inside", "keep"])
def test_converter_on_the_device_equals_the_host_run(tmp_path, fit):
    dense = synthetic_scene(tmp_path / "scene")
    host = M.convert(dense, device="cpu", undistort=True, undistort_fit=fit, write=False)
    dev = M.convert(dense, device=DEV, undistort=True, undistort_fit=fit, write=False)
    assert sorted(host) == sorted(dev)
    for key in ("intrinsics", "intrinsics_source", "extrinsics", "depth_ranges", "zoom"):
        assert np.array_equal(host[key], dev[key]), key
    for key in ("images", "masks", "valid"):                                   # a polynomial model: no atan, bytes are equal
        assert len(host[key]) == len(dev[key]) == 3
        for a, b in zip(host[key], dev[key]):
            assert a.dtype == np.uint8 and np.array_equal(a, b), key
    assert host["cam_texts"] == dev["cam_texts"] and host["names"] == dev["names"]
    # the pair kernel adds a pair's 40 positive terms in its own order (include/ufr.h): each of the at most 40 additions of either
    # order rounds by at most 2^-53 of a partial sum, which the total bounds
    assert np.allclose(host["score"], dev["score"], rtol=2 * 40 * 2.0 ** -53, atol=0)
