"""Benchmark of depth-map fusion (uforecon_amd/depth_fusion.py) on synthetic 512x640 frames: the default run of the
reference script (3 views, each against the other two) and its --full_fusion shape (49 views x 10 sources).  Per scan:
  * kernels: HIP events around every launch (ufr_profile_*), summed per stage -- consistency, compaction (count + scan,
    emit);
  * host: forming the pair matrices in numpy (perf_counter), and uploading depth maps, colours and matrix tables (HIP
    events around the copies);
  * end to end: ``fuse_views`` wall time, which adds the per-view synchronisations and the copy of the cloud to the host;
  * baseline: the numpy restatement (tests/depth_fusion_ref.py) on the same inputs, wall time on the same host.  numpy runs
    it on one thread for all practical purposes (element-wise work and 3xN products), however many CPUs the host has.
Prints one JSON line per shape; --out writes the list to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_fusion_ref as R  # noqa: E402
from uforecon_amd import depth_fusion as DF, ops  # noqa: E402


def scene(n_views, n_src, H=512, W=640, seed=0):
    """cameras on an arc in front of a wavy wall, float32 cameras as the model writes them; depth errors and holes so that
    every branch of the consistency check does work"""
    rng = np.random.default_rng(seed)
    depths, Ks, Es, colors = [], [], [], []
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v in range(n_views):
        ang = 0.012 * (v - (n_views - 1) / 2)
        c, s = np.cos(ang), np.sin(ang)
        Rm = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        eye = np.array([-6.0 * s, 0.01 * (v % 7), -6.0 * c])
        E = np.eye(4)
        E[:3, :3] = Rm
        E[:3, 3] = -Rm @ eye
        K = np.array([[2.2 * W, 0, (W - 1) / 2], [0, 2.2 * W, (H - 1) / 2], [0, 0, 1.0]])
        rays = Rm.T @ (np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)]))
        z = (-eye[2] / rays[2]).reshape(H, W)
        z = z * (1 + 0.003 * np.sin(xs / 40.0 + v) * np.cos(ys / 30.0))
        z = z * (1 + np.where(rng.random((H, W)) < 0.2, 0.01 * rng.standard_normal((H, W)), 0))
        z[rng.random((H, W)) < 0.02] = 0
        depths.append(z.astype(np.float32))
        Ks.append(K.astype(np.float32))
        Es.append(E.astype(np.float32))
        colors.append(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
    pairs = []
    for v in range(n_views):
        near = sorted((u for u in range(n_views) if u != v), key=lambda u: (abs(u - v), u))[:n_src]
        pairs.append((v, near))
    return depths, Ks, Es, colors, pairs


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def measure(n_views, n_src, baseline=True, verbose=False):
    depths, Ks, Es, colors, pairs = scene(n_views, n_src)
    kw = dict(geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2)
    DF.fuse_views(depths[:3], Ks, Es, colors, [(0, [1, 2])], **kw)             # warm: library, allocator
    # host: pair matrices
    t0 = time.perf_counter()
    mats = [np.stack([DF.pair_matrices(Ks[r], Es[r], Ks[s], Es[s]) for s in ss]) for r, ss in pairs]
    inv = [(np.linalg.inv(Ks[r]), np.linalg.inv(Es[r])) for r, _ in pairs]
    host_mats_ms = (time.perf_counter() - t0) * 1e3
    # uploads
    upload_ms, dev = _event_ms(lambda: ([torch.from_numpy(d).cuda() for d in depths], [torch.from_numpy(c).cuda() for c in colors],
                                        [torch.from_numpy(m).cuda() for m in mats]))
    d_depth, d_color, d_mats = dev
    # kernels, stage by stage
    ops.profile_enable(True)
    n_points = 0
    for i, (r, ss) in enumerate(pairs):
        _, mask, avg = ops.depth_consistency(d_depth[r], [d_depth[s] for s in ss], d_mats[i], **kw)
        xyz, _ = ops.depth_points(mask, avg, d_color[r], *inv[i])
        n_points += len(xyz)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    stage = {k: prof[k]["ms"] for k in ("depth_consistency", "depth_points_count", "depth_points_emit")}
    # end to end
    t0 = time.perf_counter()
    xyz, rgb, masks = DF.fuse_views(depths, Ks, Es, colors, pairs, **kw)
    torch.cuda.synchronize()
    end_to_end_ms = (time.perf_counter() - t0) * 1e3
    assert len(xyz) == n_points
    res = dict(shape=f"{n_views} views x {n_src} sources", image="512x640", pairs=sum(len(s) for _, s in pairs), points=n_points,
               kept=float(np.mean([m.mean() for m in masks])), consistency_ms=stage["depth_consistency"],
               compaction_ms=stage["depth_points_count"] + stage["depth_points_emit"], host_matrices_ms=host_mats_ms,
               upload_ms=upload_ms, gpu_end_to_end_ms=end_to_end_ms)
    if baseline:
        t0 = time.perf_counter()
        want = R.fuse_views(depths, Ks, Es, colors, pairs, **kw)
        res["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        res["numpy_over_gpu"] = res["numpy_ms"] / end_to_end_ms
        res["numpy_threads"] = "effectively 1"
        res["numpy_points"] = len(want[0])
    if verbose:
        print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-baseline", action="store_true", help="skip the numpy restatement (minutes at 49 x 10)")
    ap.add_argument("--out", help="write the results as JSON here")
    a = ap.parse_args()
    results = [measure(3, 2, not a.no_baseline, verbose=True), measure(49, 10, not a.no_baseline, verbose=True)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
