"""The scan loader's two kernels (csrc/frame_input.hip) against their host forms (uforecon_amd/host_forms.py), the loader on the
device against the golden batches, and the extract_geometry command end to end on the golden scan."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dtu_scan_golden as G
from uforecon_amd import _lib, host_forms as D, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# components of a unit vector lie in [-1, 1], where float32 values are at most 2^-23 = 1.19e-7 apart; the kernel and the host
# may differ by a few float64 ulps before the cast, so by one float32 step and no more
RAY_ATOL = 1.2e-7
ERR_ARG = -1                    # UFR_ERR_ARG (include/ufr.h)
RAY_DIFFERING_SHARE = 0.01      # more components than this differing at all: the kernel is not computing in double


def _rays_close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst, share = float(np.abs(got - want).max()), float((got != want).mean())
    print(f"{what}: max |delta| {worst:.3e}, differing share {share:.5f}")
    assert worst <= RAY_ATOL, (what, worst)
    assert share <= RAY_DIFFERING_SHARE, (what, share)


# ------------------------------------------------------------------ the resize kernel
@pytest.mark.parametrize("n,src,dst,clip", [
    (1, (60, 128), (32, 64), (0, 0, 0, 0)),      # DTU's factors: 1.875 and 2
    (1, (60, 128), (30, 64), (0, 0, 0, 0)),      # 2 and 2: the box mean
    (1, (7, 5), (3, 2), (0, 0, 0, 0)),
    (1, (33, 47), (32, 40), (0, 0, 0, 0)),       # odd sizes, 1280 pixels: not a multiple of the block
    (3, (60, 128), (32, 64), (4, 2, 4, 2)),      # several images and a clip
    (2, (60, 128), (30, 64), (3, 1, 5, 2)),      # the box mean under an uneven clip
    (2, (5, 6), (11, 13), (0, 0, 0, 0)),         # an enlargement: taps clamped at every edge
])
def test_resize_kernel_equals_host_form(n, src, dst, clip):
    rng = np.random.default_rng(hash((n, src, dst)) % 2 ** 32)
    imgs = rng.integers(0, 256, (n, src[0], src[1], 3), dtype=np.uint8)
    got = ops.image_resize_u8(torch.from_numpy(imgs).to(DEV), dst[0], dst[1], clip).cpu().numpy()
    want = D.image_planes_host(imgs, dst[0], dst[1], clip)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got, want), float(np.abs(got - want).max())


# ------------------------------------------------------------------ the ray kernel
@pytest.mark.parametrize("H,W", [(2, 2), (32, 64), (33, 47)])
@pytest.mark.parametrize("with_origin", [True, False])
def test_ray_kernel_equals_host_form(H, W, with_origin):
    g = G.golden_batch("set0", 1)
    m = g["ref_pose_inv"][0]
    origin = g["ray_o"][0] if with_origin else None
    got = ops.pixel_rays(m, H, W, origin, DEV).cpu().numpy()
    want = D.pixel_rays_host(m, H, W, origin).numpy()
    assert got.dtype == np.float32 and np.allclose(np.linalg.norm(got.astype(np.float64), axis=0), 1, atol=1e-6)
    _rays_close(got, want, f"rays {H}x{W} origin={with_origin}")


# ------------------------------------------------------------------ argument errors
def test_argument_errors_and_the_next_valid_call():
    lib = _lib.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    m = np.ascontiguousarray(G.golden_batch("set0", 0)["ref_pose_inv"][0])
    mp = m.ctypes.data_as(fp)
    dirs = torch.empty(3, 12, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for H, W, out in ((1, 12, dirs.data_ptr()), (12, 1, dirs.data_ptr()), (3, 4, None)):
        assert lib.ufr_pixel_rays(mp, None, H, W, out, stream) == ERR_ARG
        assert b"ufr_pixel_rays" in lib.ufr_last_error()
    assert lib.ufr_pixel_rays(None, None, 3, 4, dirs.data_ptr(), stream) == ERR_ARG
    assert lib.ufr_pixel_rays(mp, None, 3, 4, dirs.data_ptr(), stream) == 0
    _rays_close(dirs.cpu().numpy(), D.pixel_rays_host(m, 3, 4).numpy(), "rays after the refused calls")

    imgs = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, 6, 8, 3), dtype=np.uint8)).to(DEV)
    dst = torch.empty(1, 3, 3, 4, device=DEV)
    call = lambda dst_p, H, W, clip: lib.ufr_image_resize_u8(imgs.data_ptr(), 1, 6, 8, H, W, (C.c_int32 * 4)(*clip), dst_p, stream)  # noqa: E731
    assert call(None, 3, 4, (0, 0, 0, 0)) == ERR_ARG and b"null" in lib.ufr_last_error()
    assert call(dst.data_ptr(), 3, 4, (2, 0, 2, 0)) == ERR_ARG and b"leaves nothing" in lib.ufr_last_error()      # the clip eats every column
    assert call(dst.data_ptr(), 3, 4, (0, 1, 0, 2)) == ERR_ARG
    assert call(dst.data_ptr(), 3, 4, (-1, 0, 0, 0)) == ERR_ARG
    assert call(dst.data_ptr(), 0, 4, (0, 0, 0, 0)) == ERR_ARG
    assert lib.ufr_image_resize_u8(None, 1, 6, 8, 3, 4, ip(), dst.data_ptr(), stream) == ERR_ARG
    assert call(dst.data_ptr(), 3, 4, (0, 0, 0, 0)) == 0
    assert np.array_equal(dst.cpu().numpy(), D.image_planes_host(imgs.cpu().numpy(), 3, 4))
    with pytest.raises(ops.UfrError):
        ops.pixel_rays(m, 1, 5, None, DEV)
    with pytest.raises(ops.UfrError):
        ops.image_resize_u8(imgs, 3, 4, (2, 0, 2, 0))


# ------------------------------------------------------------------ the loader on the device
@pytest.fixture(scope="module")
def scan_dir(tmp_path_factory):
    return G.write_scan(tmp_path_factory.mktemp("dtu"))


@pytest.mark.parametrize("case", ["set0", "set1"])
def test_device_loader_against_the_host_loader_and_the_golden_batches(scan_dir, case):
    """The device loader against the host loader of the same machine: images equal, rays within the kernel's bound, everything
    else equal bit for bit (both ran the same host code).  Against the golden batches: images equal, and the entries that went
    through LAPACK / BLAS within the bounds of tests/dtu_scan_golden.py (another machine's libraries round them differently:
    DESIGN 3.4.4); the rays then carry the kernel's bound on top of what those entries moved them by."""
    scan, host = G.open_scan(*scan_dir, case, DEV), G.open_scan(*scan_dir, case, "cpu")
    for i, batch in enumerate(scan):
        assert all(t.device == torch.device(DEV) for k, t in batch.items() if torch.is_tensor(t))
        assert all(t.device == torch.device(DEV) for t in batch["proj_matrices"].values())
        got, same, want = G.flat_batch(batch), G.flat_batch(host[i]), G.golden_batch(case, i)
        assert set(got) == set(same) == set(want)
        for k in want:
            if k == "meta":
                assert got[k] == same[k] == want[k]
                continue
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            if k in G.RAY_KEYS:
                _rays_close(got[k], same[k], f"{case}/{i}/{k} against the host loader")
            else:
                assert np.array_equal(got[k], same[k]), (case, i, k)
        G.assert_matches_golden(got, want, f"{case}/{i}", ray_atol=RAY_ATOL)


# ------------------------------------------------------------------ the command, end to end
def _args():   # the smallest frame of tests/test_pipeline.py: 32x64, 3 views, 64 + 64 samples
    return argparse.Namespace(extract_geometry=True, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64,
                              fine_sample=64, volume_type="correlation", volume_reso=96, mvs_depth_guide=1,
                              depth_pos_encoding=True, use_dir_srdf=False, explicit_similarity=True,
                              test_coarse_only=False, test_ray_num=800, test_n_view=3, out_dir=None)


def test_command_writes_the_reference_tree(scan_dir, tmp_path):
    from uforecon_amd import depth_fusion, extract_geometry as E, pipeline, tsdf
    from uforecon_amd.scene import fill_state_dict

    root, scan = scan_dir
    g = G.golden()
    number = int(scan[4:])
    net = fill_state_dict(pipeline.UFOReconInference(_args()), 21).eval()
    ckpt = str(tmp_path / "model.ckpt")
    torch.save({"state_dict": net.state_dict()}, ckpt)
    cfg = G.cases()["set0"]
    argv = ["--test_dir", root, "--load_ckpt", ckpt, "--scans", str(number), "--set", "0", "--test_n_view", "3",
            "--test_ref_view", *[str(v) for v in cfg["test_view_pair"]], "--volume_type", "correlation", "--depth_pos_encoding",
            "--mvs_depth_guide", "1", "--explicit_similarity", "--test_ray_num", "800", "--test_sample_coarse", "64",
            "--test_sample_fine", "64", "--img_wh", *[str(v) for v in cfg["img_wh"]],
            "--original_img_wh", *[str(int(v)) for v in g["original_img_wh"]], "--seed", "5"]
    outs = [str(tmp_path / "out_a"), str(tmp_path / "out_b")]
    for out in outs:
        assert E.main(argv + ["--out_dir", out]) == 0
    net = net.to(DEV)
    host = G.open_scan(root, scan, "set0", "cpu")
    for i in range(3):
        name = "%08d" % i
        for path in (os.path.join("depth", scan, name + ".npy"), os.path.join("rgb", scan, name + ".jpg"),
                     os.path.join(scan, "depth", name + ".png")):
            assert os.path.exists(os.path.join(outs[0], path)), path
        raw = [open(os.path.join(o, "depth", scan, name + ".npy"), "rb").read() for o in outs]
        assert raw[0] == raw[1], f"view {i}: a rerun with the same --seed wrote another file"
        d = np.load(os.path.join(outs[0], "depth", scan, name + ".npy"), allow_pickle=True).item()
        ref = G.flat_batch(host[i])                      # the reference batch as this machine's host code computes it
        assert d["depth"].shape == (32, 64) and d["depth"].dtype == np.float32 and np.isfinite(d["depth"]).all()
        assert np.array_equal(d["extrinsic"], ref["extrinsic_render_view"][0])
        assert np.array_equal(d["intrinsic"], ref["intrinsic_render_view"][0])
        # that batch through the same model and uniforms: tests/test_pipeline.py compares its depth maps with np.array_equal,
        # so this does too
        uniforms = E.view_uniforms(5, number, i, 64, 64, 32 * 64)
        depths, _ = net.extract_geometry(G.to_device(host[i], DEV), uniforms=uniforms)
        print(f"view {i}: max |depth - depth of the host loader's batch| {float(np.abs(d['depth'] - depths).max()):.3e} "
              f"at a depth of about {float(np.median(depths)):.1f}; differing pixels {int((d['depth'] != depths).sum())}")
        assert np.array_equal(d["depth"], depths)
        # ... and the golden batch itself, whose cameras another machine's LAPACK rounded: a figure, and a loose bound on the
        # typical pixel (a relative 1e-6 in the cameras moves a sample by as much; three decades are left for the network)
        want = G.golden_batch("set0", i)
        batch = {k: torch.from_numpy(v).to(DEV) for k, v in want.items() if k != "meta" and not k.startswith("proj_matrices.")}
        batch["proj_matrices"] = {st: torch.from_numpy(want["proj_matrices." + st]).to(DEV) for st in ("stage1", "stage2", "stage3")}
        batch["meta"] = [want["meta"]]
        depths_g, _ = net.extract_geometry(batch, uniforms=uniforms)
        rel = np.abs(d["depth"] - depths_g) / np.abs(depths_g)
        print(f"view {i}: against the golden batch: median relative departure {float(np.median(rel)):.3e}, max {float(rel.max()):.3e}, "
              f"differing pixels {int((d['depth'] != depths_g).sum())}")
        assert float(np.median(rel)) < 1e-3
    # the tree is what the fusion commands read.  depth_fusion takes the `%08d` names; tsdf.save_tsdf looks for the
    # `refview<i>` names of the reference's tsdf_fusion.py, finds none and ends in its orderly empty-volume error, so the
    # files are also fused the way save_tsdf reads them (np.load(...).item(), tests/test_pipeline.py)
    xyz, rgb, masks = depth_fusion.filter_depth(outs[0], scan, n_view=3)
    assert len(masks) == 3 and xyz.shape[1:] == (3,) and len(xyz) == len(rgb)
    try:
        V, F = tsdf.save_tsdf(outs[0], scan, voxel_size=10.0)
        assert V >= 0 and F >= 0
    except ops.UfrError as e:
        assert "unsupported" in str(e)
    frames = [np.load(os.path.join(outs[0], "depth", scan, "%08d.npy" % i), allow_pickle=True).item() for i in range(3)]
    vol = tsdf.fuse_depth_maps([f["depth"] for f in frames], [f["intrinsic"] for f in frames], [f["extrinsic"] for f in frames],
                               voxel_size=10.0, margin=3)
    t, _, w = vol.get_volume()
    assert (w > 0).sum() > 100 and np.isfinite(t).all()
    for i in range(3):       # what was rendered is the golden batch, up to the rounding of this machine's LAPACK
        G.assert_matches_golden(G.flat_batch(host[i]), G.golden_batch("set0", i), f"set0/{i}")
