"""The masked image kernel (csrc/frame_input.hip, ufr_image_resize_mask_u8) against its host form, the custom-scene loader on
the device against the host loader and the golden batches, the extract_geometry command with --test_general end to end, and
the converter's output read by the loader."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dtu_scan_golden as G
import general_scan_golden as S
from test_gpu_dtu_scan import RAY_ATOL, _rays_close
from uforecon_amd import _lib, general_scan as GS, host_forms as D, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1


# ------------------------------------------------------------------ the masked resize kernel
@pytest.mark.parametrize("n,src,dst,clip", [
    (1, (60, 128), (32, 64), (0, 0, 0, 0)),      # general factors: 1.875 and 2
    (1, (60, 128), (30, 64), (0, 0, 0, 0)),      # exactly 2 and 2: the box mean
    (3, (60, 128), (32, 64), (4, 2, 4, 2)),      # several images and a clip
    (3, (60, 128), (30, 64), (3, 1, 5, 2)),      # the box mean under an uneven clip
    (1, (33, 47), (32, 40), (0, 0, 0, 0)),       # odd sizes, 1280 pixels: not a multiple of the block
    (1, (5, 6), (11, 13), (0, 0, 0, 0)),         # an enlargement: taps clamped at every edge
])
def test_masked_resize_kernel_equals_host_form(n, src, dst, clip):
    rng = np.random.default_rng(hash((n, src, dst)) % 2 ** 32)
    imgs = rng.integers(0, 256, (n, src[0], src[1], 3), dtype=np.uint8)
    masks = rng.choice(np.array([0, 254, 255, 128], np.uint8), (n, src[0], src[1]), p=[0.3, 0.3, 0.3, 0.1])
    imgs[0, :2, :2], masks[0, :2, :2] = 255, 255                  # 255 x 255: slightly more than 1 (the reference's 254)
    got = ops.image_resize_mask_u8(torch.from_numpy(imgs).to(DEV), torch.from_numpy(masks).to(DEV), dst[0], dst[1], clip).cpu().numpy()
    want = D.image_mask_planes_host(imgs, masks, dst[0], dst[1], clip)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    full = ops.image_resize_mask_u8(torch.from_numpy(imgs).to(DEV), torch.full(masks.shape, 254, dtype=torch.uint8, device=DEV), dst[0], dst[1], clip)
    assert torch.equal(full, ops.image_resize_u8(torch.from_numpy(imgs).to(DEV), dst[0], dst[1], clip))      # 254 = all of it


def test_masked_resize_argument_errors_and_the_next_valid_call():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    imgs = torch.from_numpy(rng.integers(0, 256, (1, 6, 8, 3), dtype=np.uint8)).to(DEV)
    masks = torch.from_numpy(rng.integers(0, 256, (1, 6, 8), dtype=np.uint8)).to(DEV)
    dst = torch.empty(1, 3, 3, 4, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda src, msk, dst_p, H, W, clip: lib.ufr_image_resize_mask_u8(src, msk, 1, 6, 8, H, W, (C.c_int32 * 4)(*clip), dst_p, stream)  # noqa: E731
    ok = (imgs.data_ptr(), masks.data_ptr(), dst.data_ptr())
    assert call(ok[0], None, ok[2], 3, 4, (0, 0, 0, 0)) == ERR_ARG and b"ufr_image_resize_mask_u8" in lib.ufr_last_error()
    assert call(None, ok[1], ok[2], 3, 4, (0, 0, 0, 0)) == ERR_ARG and b"null" in lib.ufr_last_error()
    assert call(ok[0], ok[1], None, 3, 4, (0, 0, 0, 0)) == ERR_ARG
    assert call(*ok, 3, 4, (2, 0, 2, 0)) == ERR_ARG and b"leaves nothing" in lib.ufr_last_error()
    assert call(*ok, 3, 4, (-1, 0, 0, 0)) == ERR_ARG
    assert call(*ok, 0, 4, (0, 0, 0, 0)) == ERR_ARG
    assert call(*ok, 3, 4, (0, 0, 0, 0)) == 0
    assert np.array_equal(dst.cpu().numpy(), D.image_mask_planes_host(imgs.cpu().numpy(), masks.cpu().numpy(), 3, 4))
    with pytest.raises(ops.UfrError):
        ops.image_resize_mask_u8(imgs, masks[:, :5], 3, 4)


# ------------------------------------------------------------------ the loader on the device
@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return S.write_scene(tmp_path_factory.mktemp("general"))


@pytest.mark.parametrize("case", ["mvimage", "blendedmvs"])
def test_device_loader_against_the_host_loader_and_the_golden_batches(scene_dir, case):
    """As tests/test_gpu_dtu_scan.py does for DtuScan: against the host loader of the same machine images equal, rays within the
    kernel's bound, everything else equal bit for bit; against the golden batches the bounds of tests/dtu_scan_golden.py."""
    scan, host = S.open_scan(*scene_dir, case, DEV), S.open_scan(*scene_dir, case, "cpu")
    assert len(scan) == len(host) == len(S.metas(case))
    for i, batch in enumerate(scan):
        assert all(t.device == torch.device(DEV) for k, t in batch.items() if torch.is_tensor(t))
        assert all(t.device == torch.device(DEV) for t in batch["proj_matrices"].values())
        got, same, want = G.flat_batch(batch), G.flat_batch(host[i]), S.golden_batch(case, i)
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


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from uforecon_amd import pipeline
    from uforecon_amd.scene import fill_state_dict

    net = fill_state_dict(pipeline.UFOReconInference(_args()), 21).eval()
    path = str(tmp_path_factory.mktemp("ckpt") / "model.ckpt")
    torch.save({"state_dict": net.state_dict()}, path)
    return path


def _argv(root, scans, ckpt, refs):
    return ["--test_dir", root, "--load_ckpt", ckpt, "--test_general", "--test_scan", *scans, "--dataset", "mvimage", "--use_mask",
            "--test_n_view", "3", "--test_ref_view", *[str(v) for v in refs], "--volume_type", "correlation", "--depth_pos_encoding",
            "--mvs_depth_guide", "1", "--explicit_similarity", "--test_ray_num", "800", "--test_sample_coarse", "64",
            "--test_sample_fine", "64", "--img_wh", "64", "32", "--seed", "5"]


def _check_tree(out, scan, refs):
    for v in refs:
        for path in (os.path.join("depth", scan, "refview%d.npy" % v), os.path.join("rgb", scan, "refview%d.jpg" % v),
                     os.path.join(scan, "depth", "refview%d.png" % v)):
            assert os.path.exists(os.path.join(out, path)), path
        d = np.load(os.path.join(out, "depth", scan, "refview%d.npy" % v), allow_pickle=True).item()
        assert sorted(d) == ["depth", "extrinsic", "intrinsic"]
        assert d["depth"].shape == (32, 64) and d["depth"].dtype == np.float32 and np.isfinite(d["depth"]).all()
        assert d["intrinsic"].shape == (3, 3) and d["intrinsic"].dtype == np.float32
        assert d["extrinsic"].shape == (4, 4) and d["extrinsic"].dtype == np.float32
    assert sorted(os.listdir(os.path.join(out, "depth", scan))) == sorted("refview%d.npy" % v for v in refs)


def test_command_with_test_general_writes_the_refview_tree(scene_dir, checkpoint, tmp_path, monkeypatch):
    from uforecon_amd import extract_geometry as E, tsdf

    root, scan = scene_dir
    refs = S.cases()["mvimage"]["test_ref_view"]
    outs = [str(tmp_path / "out_a"), str(tmp_path / "out_b")]
    for out in outs:
        assert E.main(_argv(root, [scan], checkpoint, refs) + ["--out_dir", out]) == 0
    _check_tree(outs[0], scan, refs)
    host = S.open_scan(root, scan, "mvimage", "cpu")
    for i, v in enumerate(refs):
        for rel in (os.path.join("depth", scan, "refview%d.npy" % v), os.path.join("rgb", scan, "refview%d.jpg" % v),
                    os.path.join(scan, "depth", "refview%d.png" % v)):
            raw = [open(os.path.join(o, rel), "rb").read() for o in outs]
            assert raw[0] == raw[1], f"{rel}: a rerun with the same --seed wrote another file"
        d = np.load(os.path.join(outs[0], "depth", scan, "refview%d.npy" % v), allow_pickle=True).item()
        ref = G.flat_batch(host[i])                      # the same batch as this machine's host code computes it
        assert np.array_equal(d["extrinsic"], ref["extrinsic_render_view"][0]) and np.array_equal(d["intrinsic"], ref["intrinsic_render_view"][0])
    # the tree is what `python -m uforecon_amd.tsdf --dataset general --test_scan <scan>` reads: save_tsdf must find every view.
    # With untrained weights the mesh may be empty or the volume refused as unsupported: the views read are what is asserted
    seen = []
    real_load = np.load
    monkeypatch.setattr(tsdf.np, "load", lambda path, *a, **kw: (seen.append(os.path.basename(str(path))), real_load(path, *a, **kw))[1])
    try:
        V, F = tsdf.save_tsdf(outs[0], scan, voxel_size=10.0)
        assert V >= 0 and F >= 0
    except ops.UfrError as e:
        assert "unsupported" in str(e)
    # (without a view list save_tsdf, like the reference, looks for refview0 .. refview<n-1>, n the number of pictures: of the
    # reference views 0, 2 and 3 it finds 0 and 2)
    assert sorted(seen) == ["refview0.npy", "refview2.npy"]
    # ... and every view by explicit list, as `--test_view 0 2 3` passes it
    del seen[:]
    try:
        tsdf.save_tsdf(outs[0], scan, test_view=refs, voxel_size=10.0)
    except ops.UfrError as e:
        assert "unsupported" in str(e)
    assert sorted(seen) == sorted("refview%d.npy" % v for v in refs)


def test_converter_output_read_by_the_loader(tmp_path, checkpoint):
    """colmap2mvsnet.convert -> GeneralScan on the converter's own output: the cams/pair.txt hand-off, the copied pictures and
    masks (PNG bytes under a .jpg name, as the reference leaves them), then one view through the command"""
    from uforecon_amd import colmap2mvsnet as M, extract_geometry as E

    dense = S.write_colmap_scene(tmp_path)
    out = M.convert(dense, device=DEV)
    root, scan = os.path.dirname(dense), os.path.basename(dense)
    for k in (1, 3, 5):                                  # the golden scene has masks for half of its pictures: the rest are all foreground
        from PIL import Image
        Image.fromarray(np.full((60, 128), 254, np.uint8)).save(os.path.join(dense, "masks", "%08d_mask.jpg" % k), format="PNG")
    ranked = [k for k, _ in out["view_sel"][2]]
    scene = GS.GeneralScan(root, scan, n_views=3, test_ref_view=[], dataset="mvimage", use_mask=True, img_wh=[64, 32], device=DEV)
    host = GS.GeneralScan(root, scan, n_views=3, test_ref_view=[], dataset="mvimage", use_mask=True, img_wh=[64, 32], device="cpu")
    assert len(scene) == 6 and scene.metas[2] == (2, ranked) and scene.view_ids(2) == [2] + ranked[:2]
    got, same = G.flat_batch(scene[2]), G.flat_batch(host[2])
    assert got["meta"] == "%s-%s-refview2" % (os.path.basename(root), scan)
    for k in same:
        if k in G.RAY_KEYS:
            _rays_close(got[k], same[k], f"converted scene: {k}")
        elif k != "meta":
            assert np.array_equal(got[k], same[k]), k
    # the depth hypotheses come from the converter's depth line of the last view read
    lo, step = out["depth_ranges"][ranked[1]][:2]
    want = np.arange(float("%f" % lo), float("%f" % step) * 1.06 * 192 + float("%f" % lo), float("%f" % step) * 1.06, dtype=np.float32)
    assert np.array_equal(got["depth_values_org_scale"][0], want)
    # the mask did something where the scene has one (view 2 has a mask file of its own)
    plain = GS.GeneralScan(root, scan, n_views=3, test_ref_view=[], dataset="mvimage", use_mask=False, img_wh=[64, 32], device=DEV)[2]
    assert not torch.equal(plain["ref_img"], scene[2]["ref_img"])
    out_dir = str(tmp_path / "out")
    assert E.main(_argv(root, [scan], checkpoint, [2, 1, 3]) + ["--out_dir", out_dir]) == 0
    _check_tree(out_dir, scan, [1, 2, 3])
