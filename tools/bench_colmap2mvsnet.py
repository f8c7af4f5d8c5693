"""Benchmark of the custom-scene route's two kernels at one stated synthetic size each:
  * the pair scores of the view selection (ufr_view_pair_scores: offsets, sort and pair kernel as one timed call, HIP events
    through ufr_profile_*) for 100 images of 2000 observations each over 20000 points -- 4950 pairs -- against the numpy host
    form `colmap2mvsnet.pair_scores_host` (wall time; vectorised per pair with np.isin, so already far faster than the
    reference's per-pair list comprehension, which is not run here);
  * the masked resize (ufr_image_resize_mask_u8) for 3 pictures of 1920 x 1080 -> 960 x 544 against its host form
    `host_forms.image_mask_planes_host`.
There is no pass mark and no earlier figure to compare with: this file records what was measured and on what.  Prints one JSON
line; --out writes it to a file (profiles/colmap2mvsnet_bench.json is one such run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uforecon_amd import colmap2mvsnet as M, host_forms as D, ops  # noqa: E402

IMAGES, OBSERVATIONS, POINTS = 100, 2000, 20000
SOURCE_HW, IMG_HW, VIEWS = (1080, 1920), (544, 960), 3


def synthetic_lists(rng):
    """every image sees a window of the points around its own place on a ring of cameras, 5 % of its observations without a point"""
    centres = np.stack([650.0 * np.array([np.sin(2 * np.pi * k / IMAGES), -np.cos(2 * np.pi * k / IMAGES), 0.3]) for k in range(IMAGES)])
    points = rng.uniform(-120, 120, (POINTS, 3))
    lists = []
    for k in range(IMAGES):
        window = (k * POINTS // IMAGES + rng.integers(0, POINTS // 4, OBSERVATIONS)) % POINTS
        window[rng.random(OBSERVATIONS) < 0.05] = -1
        lists.append(window.astype(np.int32))
    offsets = np.arange(IMAGES + 1, dtype=np.int64) * OBSERVATIONS
    return offsets, np.concatenate(lists), points, centres


def best_ms(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_repeats", type=int, default=1, help="repeats of the host score form (seconds each)")
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, images=IMAGES, observations_per_image=OBSERVATIONS, points=POINTS,
               pairs=IMAGES * (IMAGES - 1) // 2, resize=f"{VIEWS} x {SOURCE_HW[0]}x{SOURCE_HW[1]} -> {IMG_HW[0]}x{IMG_HW[1]}",
               timing="kernels by HIP events, mean over the repeats; host forms and wall times best of the repeats")
    offsets, obs, points, centres = synthetic_lists(rng)
    d_points, d_centres = torch.from_numpy(points).to(dev), torch.from_numpy(centres).to(dev)
    got = ops.view_pair_scores(offsets, obs, d_points, d_centres, device=dev)            # warm: library, allocator
    torch.cuda.synchronize()
    ops.profile_enable(True)
    for _ in range(a.repeats):
        ops.view_pair_scores(offsets, obs, d_points, d_centres, device=dev)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    res["score_kernels_ms"] = prof["view_pair_scores"]["ms"] / a.repeats
    res["score_call_wall_ms"] = best_ms(lambda: (ops.view_pair_scores(offsets, obs, d_points, d_centres, device=dev), torch.cuda.synchronize()),
                                        a.repeats)
    host = [None]
    res["score_host_ms"] = best_ms(lambda: host.__setitem__(0, M.pair_scores_host(offsets, obs, points, centres)), a.host_repeats)
    res["score_max_rel_diff"] = float(np.abs(got.cpu().numpy() - host[0]).max() / host[0].max())
    res["mean_shared_observations_per_pair"] = float(np.mean([np.isin(obs[offsets[i]:offsets[i + 1]], obs[offsets[i + 1]:offsets[i + 2]]).sum()
                                                              for i in range(IMAGES - 1)]))

    yy, xx = np.mgrid[0:SOURCE_HW[0], 0:SOURCE_HW[1]]
    raw = np.stack([np.stack([127 + 100 * np.sin(xx / (40.0 + 9 * c) + k) * np.cos(yy / (55.0 - 7 * c)) for c in range(3)], -1) for k in range(VIEWS)])
    raw = np.clip(raw + rng.normal(0, 4, raw.shape), 0, 255).astype(np.uint8)
    masks = np.where((yy - SOURCE_HW[0] / 2) ** 2 + (xx - SOURCE_HW[1] / 2) ** 2 < (SOURCE_HW[0] / 2.2) ** 2, 255, 0).astype(np.uint8)
    masks = np.ascontiguousarray(np.broadcast_to(masks, (VIEWS,) + masks.shape))
    d_raw, d_masks = torch.from_numpy(raw).to(dev), torch.from_numpy(masks).to(dev)
    out = ops.image_resize_mask_u8(d_raw, d_masks, *IMG_HW)
    torch.cuda.synchronize()
    ops.profile_enable(True)
    for _ in range(a.repeats):
        ops.image_resize_mask_u8(d_raw, d_masks, *IMG_HW)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    res["masked_resize_kernel_ms"] = prof["image_resize_mask_u8"]["ms"] / a.repeats
    want = [None]
    res["masked_resize_host_ms"] = best_ms(lambda: want.__setitem__(0, D.image_mask_planes_host(raw, masks, *IMG_HW)), a.repeats)
    res["masked_resize_equal"] = bool(np.array_equal(out.cpu().numpy(), want[0]))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
