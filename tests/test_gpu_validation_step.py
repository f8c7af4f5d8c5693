"""UFOReconInference.validation_step / validation_epoch_end (code1/model.py:578-758) on a synthetic train-layout frame: the
hand-offs (encoder -> both passes -> scores -> files), not reference numbers -- each stage has its own parity test."""
import argparse

import numpy as np
import pytest
import torch

import frame_metrics_ref as R
from helpers import load_weights
from uforecon_amd import ops, pipeline
from uforecon_amd._lib import UfrError
from uforecon_amd.scene import fill_state_dict, make_frame, sampler_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, NV = 32, 64, 3
META = "scan24_light3_refview23"


def _args():
    return argparse.Namespace(extract_geometry=False, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64,
                              fine_sample=64, volume_type="correlation", volume_reso=96, mvs_depth_guide=1,
                              depth_pos_encoding=True, use_dir_srdf=False, explicit_similarity=True,
                              test_coarse_only=False, train_ray_num=1024, test_n_view=NV, train_n_view=NV + 1, logdir=None)


def _batch(seed=0):
    """A train-layout batch (dtu_train.py:442-495): the reference view first in w2cs / intrinsics / near_fars, ref_img,
    depths_h, no start_idx; plus what the encoder half reads."""
    fr = make_frame(H, W, NV, seed=seed, train_layout=True).to(DEV)
    batch = fr.batch
    pm = {}
    for st, s in (("stage1", 4), ("stage2", 2), ("stage3", 1)):
        p = torch.zeros(1, NV, 2, 4, 4, device=DEV)
        p[0, :, 0] = batch["w2cs"][0, 1:]
        K = batch["intrinsics"][0, 1:].clone()
        K[:, :2] = K[:, :2] / s
        p[0, :, 1, :3, :3] = K
        p[0, :, 1, 3, 3] = 1.0
        pm[st] = p
    batch["proj_matrices"] = pm
    near, far = float(batch["near_fars"][0, 0, 0]), float(batch["near_fars"][0, 0, 1])
    batch["depth_values_org_scale"] = torch.linspace(near, far, 48, device=DEV)[None]
    batch["scale_mat"] = torch.diag(torch.tensor([1.5, 1.5, 1.5, 1.0], device=DEV))[None]
    batch["meta"] = [META]
    # ground-truth depth with holes and values outside near / far
    gt = batch["depths_h"][0, 0]
    gt[::5, ::3] = 0.0
    gt[1, :] = far + 0.5
    return batch


@pytest.fixture(scope="module")
def net():
    n = fill_state_dict(pipeline.UFOReconInference(_args(), tune_convolutions=False), 21).eval().to(DEV)
    n.load_state_dict(load_weights(), strict=False)
    return n


@pytest.fixture(scope="module")
def frame(net, tmp_path_factory):
    logdir = tmp_path_factory.mktemp("val")
    batch = _batch()
    U = sampler_uniforms(11, 64, 64, H * W)
    result = net.validation_step(batch, 0, logdir=str(logdir), uniforms=U)
    return batch, U, result, logdir


def _render(net, batch, U):
    feat, vols, match = net.encode_frame(batch, cur_n_src_views=NV)
    fh = net.frame_handle({k: v for k, v in batch.items() if k != "cam_ray_d"}, feat, vols, match)
    return ops.render_rays(fh, net._weights(), torch.arange(H * W, device=DEV), U[0].to(DEV), U[1].to(DEV), want_srdf=False,
                           pair=True)


def test_returned_scores_are_those_of_the_pair_render(net, frame):
    batch, U, result, _ = frame
    out = _render(net, batch, U)
    nf = batch["near_fars"][0, 0]
    want = R.frame_metrics(out["rgb_coarse"], out["rgb"], batch["ref_img"][0], out["depth_coarse"], out["depth"],
                           batch["depths_h"][0, 0], float(nf[0]), float(nf[1]))
    assert 0 < want[6] < H * W                     # some pixels valid, some not
    assert set(result) == set(R.KEYS) | {"val/variance"}
    for i, k in enumerate(R.KEYS):
        assert isinstance(result[k], float) and np.isfinite(result[k])
        assert abs(result[k] - want[i]) <= 1e-9 * abs(want[i]), (k, result[k], want[i])
    v = result["val/variance"]
    assert v.shape == (1, 1) and abs(v.item() - float(np.exp(-10.0 * float(net.deviation_network.variance.detach())))) < 1e-6 * v.item()


def test_files_are_the_references(net, frame):
    from PIL import Image

    batch, U, _, logdir = frame
    out = _render(net, batch, U)
    png, jpg, npy = logdir / "scan24" / "depth" / "refview23.png", logdir / "rgb" / "scan24" / "refview23.jpg", \
        logdir / "depth" / "scan24" / "refview23.npy"
    assert png.exists() and jpg.exists() and npy.exists()
    scale = batch["scale_mat"][0][0, 0]
    d = np.load(npy, allow_pickle=True).item()
    want_depth = (out["depth_coarse"].view(H, W) * scale).cpu().numpy()       # the COARSE ray-length depth, scaled back
    assert d["depth"].dtype == np.float32 and np.array_equal(d["depth"], want_depth)
    assert np.array_equal(d["extrinsic"], batch["w2cs"][0][0].cpu().numpy())
    assert np.array_equal(d["intrinsic"], batch["intrinsics"][0][0].cpu().numpy())
    rgb8, depth8 = ops.frame_preview_u8(out["rgb"], out["depth_coarse"], out["depth_coarse"].max().double().reshape(1), float(scale))
    assert np.array_equal(np.array(Image.open(png)), depth8.view(H, W).cpu().numpy())
    want_rgb8, want_depth8 = R.preview_u8(out["rgb"], out["depth_coarse"], float(scale))      # ... and numpy's own bytes
    assert np.array_equal(depth8.cpu().numpy(), want_depth8) and np.array_equal(rgb8.cpu().numpy(), want_rgb8)
    assert np.array(Image.open(jpg)).shape == (H, W, 3)                       # the FINE colour, lossy


def test_rerun_gives_the_same_dict(net, frame):
    _, U, result, _ = frame
    again = net.validation_step(_batch(), 0, uniforms=U)
    assert {k: result[k] for k in R.KEYS} == {k: again[k] for k in R.KEYS}


def test_batch_of_two_is_refused(net):
    b = _batch()
    b["source_imgs"] = b["source_imgs"].expand(2, -1, -1, -1, -1)
    with pytest.raises(UfrError, match="B=1"):
        net.validation_step(b)


def test_epoch_end_is_the_mean(net, frame):
    _, _, result, _ = frame
    other = net.validation_step(_batch(seed=1), 0, uniforms=sampler_uniforms(12, 64, 64, H * W))
    end = net.validation_epoch_end([result, other])
    for src, dst in (("psnr/coarse", "psnr/coarse"), ("psnr/fine", "psnr/fine"), ("val/loss_rgb_coarse", "val/rgb_coarse"),
                     ("val/loss_rgb_fine", "val/rgb_fine"), ("val/loss_depth_coarse", "val/loss_depth_coarse"),
                     ("val/loss_depth_fine", "val/loss_depth_fine")):
        assert end[dst] == (result[src] + other[src]) / 2
        assert result[src] != other[src]
    assert end["loss"] == end["val/rgb_coarse"] + end["val/rgb_fine"]
