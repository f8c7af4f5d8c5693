"""Benchmark of the validation path on one 512x640 frame of the synthetic DTU training tree (tests/dtu_train_golden.py), 3 source
views, 64 + 64 samples.  Each new path against its counterpart:
  * loader: `DtuTrain(device="cuda")`'s first batch (wall time, files included), and the depth kernel (`ufr_depth_gt_prepare`, HIP
    events, upload of the PFM rows excluded) against its host form `depth_gt_host` (wall time);
  * scores: `ufr_frame_metrics` + `ufr_frame_preview_u8` against the same scores and bytes through torch ops on the GPU (HIP
    events around both);
  * frame: `validation_frame` (the per-ray half of `validation_step`: one `ufr_render_rays_pair` call, the metrics kernels, one
    small copy) against the route there was before it -- `infer(extract_geometry=False)` under `no_grad` in chunks of
    `train_ray_num` rays plus torch metrics -- wall time after a synchronise; both leave the encoder out, which
    `validation_step_ms` adds;
  * pair: `ops.render_rays(pair=True)` against `ops.render_rays` over the whole frame (HIP events, best of `--reps`).
Prints one JSON object; --out writes it to a file."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dtu_train_golden as G  # noqa: E402
from helpers import load_weights  # noqa: E402
from uforecon_amd import ops, pipeline  # noqa: E402
from uforecon_amd.dtu_train import PFM_CROP, depth_gt_host, read_pfm_rows  # noqa: E402
from uforecon_amd.scene import fill_state_dict, sampler_uniforms  # noqa: E402

DEV = "cuda:0"


def _event_ms(fn, reps=1):
    best, out = float("inf"), None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best, out


def _wall_ms(fn, reps=1):
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def torch_scores(rgb_c, rgb_f, ref_img, depth_c, depth_f, depth_gt, near, far, scale):
    """model.py:708-742 through torch ops on the GPU (piq.psnr as its formula)"""
    gt = ref_img.reshape(3, -1).t()
    psnr = lambda x: -10.0 * torch.log10(F.mse_loss(x.clamp(0, 1), gt.clamp(0, 1)) + 1e-8)  # noqa: E731
    g = depth_gt.reshape(-1)
    m = (g != 0) & (g >= near) & (g <= far)
    vals = [F.mse_loss(rgb_c, gt), F.mse_loss(rgb_f, gt), psnr(rgb_c), psnr(rgb_f), F.l1_loss(depth_c[m], g[m]), F.l1_loss(depth_f[m], g[m])]
    rgb8 = (rgb_f * 255).to(torch.uint8)
    d = depth_c * scale
    depth8 = ((d / d.max()) * 255).to(torch.uint8)
    return torch.stack(vals).cpu(), rgb8, depth8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    res = dict(image="512x640", source_views=3, samples="64+64", device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        root = G.write_tree(tmp)
        i = G.items()["test"][1]
        ops.pixel_rays(np.eye(4, dtype=np.float32), 8, 8, None, DEV)                     # warm: library, allocator
        res["loader_first_batch_ms"], batch = _wall_ms(lambda: G.open_dataset(root, "test", DEV)[i])
        res["loader_next_batch_ms"], _ = _wall_ms(lambda: G.open_dataset(root, "test", DEV)[i])
        scan, _, view, _ = G.metas("test")[i]
        rows, bottom_up = read_pfm_rows(os.path.join(root, "Depths_raw", scan, "depth_map_%04d.pfm" % view))
    H, W = batch["source_imgs"].shape[-2:]
    HW = H * W
    sf = float(batch["scale_factor"][0])
    z64 = torch.rand(HW, dtype=torch.float64, device=DEV) * 0.2 + 0.8
    d_rows = torch.from_numpy(rows).to(DEV)
    res["depth_kernel_ms"], got = _event_ms(lambda: ops.depth_gt_prepare(d_rows, bottom_up, *PFM_CROP, H, W, sf, z64), a.reps)
    z_host = z64.cpu().numpy()
    t0 = time.perf_counter()
    want = depth_gt_host(rows, bottom_up, *PFM_CROP, H, W, sf, z_host)
    res["depth_host_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(got.cpu().numpy(), want)
    res["depth_host_over_kernel"] = res["depth_host_ms"] / res["depth_kernel_ms"]

    args = argparse.Namespace(extract_geometry=False, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64, fine_sample=64,
                              volume_type="correlation", volume_reso=96, mvs_depth_guide=1, depth_pos_encoding=True, use_dir_srdf=False,
                              explicit_similarity=True, test_coarse_only=False, train_ray_num=1024, test_n_view=3, train_n_view=4, logdir=None)
    net = fill_state_dict(pipeline.UFOReconInference(args), 21).eval().to(DEV)
    net.load_state_dict(load_weights(), strict=False)
    U = sampler_uniforms(11, 64, 64, HW)
    net.validation_step(batch, 0, uniforms=U)                                              # warm: convolution search, workspaces
    res["validation_step_ms"], _ = _wall_ms(lambda: net.validation_step(batch, 0, uniforms=U), 3)
    feat, vols, match = net.encode_frame(batch, cur_n_src_views=3)
    res["validation_frame_ms"], new = _wall_ms(lambda: net.validation_frame(batch, feat, vols, match, uniforms=U), a.reps)

    # the pair render against the one-pass-out render, whole frame
    fh = net.frame_handle({k: v for k, v in batch.items() if k != "cam_ray_d"}, feat, vols, match)
    Wt, idx = net._weights(), torch.arange(HW, device=DEV)
    u1, u2 = U[0].to(DEV), U[1].to(DEV)
    ws = ops.RenderWorkspace(DEV, 64, 64, fh.NV)
    fh_z = net.frame_handle(batch, feat, vols, match)
    res["render_pair_ms"], out = _event_ms(lambda: ops.render_rays(fh, Wt, idx, u1, u2, workspace=ws, want_srdf=False, pair=True), a.reps)
    res["render_rays_ms"], _ = _event_ms(lambda: ops.render_rays(fh_z, Wt, idx, u1, u2, workspace=ws, want_srdf=False), a.reps)
    res["pair_over_render_rays"] = res["render_pair_ms"] / res["render_rays_ms"]

    # the scores: kernels against torch ops on the same tensors
    ref_img, gt = batch["ref_img"][0].contiguous(), batch["depths_h"][0, 0].contiguous()
    scale = float(batch["scale_mat"][0][0, 0])

    def kernels():
        o8 = ops.frame_metrics(out["rgb_coarse"], out["rgb"], ref_img, out["depth_coarse"], out["depth"], gt, fh.near_z, fh.far_z)
        return o8.cpu(), ops.frame_preview_u8(out["rgb"], out["depth_coarse"], o8[7:8], scale)

    def torch_ops():
        return torch_scores(out["rgb_coarse"], out["rgb"], ref_img, out["depth_coarse"], out["depth"], gt, fh.near_z, fh.far_z, scale)

    kernels(), torch_ops()
    res["metrics_kernels_ms"], k = _event_ms(kernels, a.reps)
    res["metrics_torch_ms"], t = _event_ms(torch_ops, a.reps)
    res["metrics_torch_over_kernels"] = res["metrics_torch_ms"] / res["metrics_kernels_ms"]
    assert torch.allclose(k[0][:6], t[0].double(), rtol=1e-4) and torch.equal(k[1][0], t[1]) and torch.equal(k[1][1], t[2])

    # the route without the pair entry: the autograd nodes under no_grad, train_ray_num rays at a time, then torch metrics
    def chunked():
        rc, rf, dc, df = [], [], [], []
        with torch.no_grad():
            for c in torch.split(idx[None], args.train_ray_num, dim=1):
                lo, hi = int(c[0, 0]), int(c[0, -1]) + 1
                r = net.infer(batch, c, feat, vols, match_feature=match, is_train=False, uniforms=(U[0][:, lo:hi], U[1][:, lo:hi]))
                rc.append(r[1][0]), dc.append(r[2][0]), rf.append(r[8][0]), df.append(r[9][0])
        return torch_scores(torch.cat(rc), torch.cat(rf), ref_img, torch.cat(dc), torch.cat(df), gt, fh.near_z, fh.far_z, scale)

    chunked()
    res["chunked_infer_frame_ms"], old = _wall_ms(chunked, 2)
    res["chunked_over_validation_frame"] = res["chunked_infer_frame_ms"] / res["validation_frame_ms"]
    res["scores"] = {k_: new[k_] for k_ in ops.FRAME_METRIC_KEYS[:6]}
    res["scores_chunked_route"] = [float(v) for v in old[0]]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
