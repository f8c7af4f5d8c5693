"""Benchmark of the undistortion kernel (ufr_image_undistort_u8, csrc/undistort.hip) at one stated size: 8 pictures of
1920 x 1080 x 3 taken by one OPENCV camera, resampled to the pinhole camera that `undistort.fit_zoom` finds, against the numpy
host form `undistort.undistort_host` on the same node -- the only earlier route to these bytes.

  kernel time   HIP events around the launch (ufr_profile_*), mean over --repeats launches after a warm-up; the pictures are
                on the device before the window opens;
  call time     host clock around the same launches ending in a synchronise, per launch;
  bytes         what the rule needs, from the shapes: every source byte once, every output byte once, the valid plane once
                (2 n H W C + H W); over the kernel time that is the achieved rate, printed beside the HBM figures of the MI355X
                (8 TB/s peak, about 6.3 TB/s achievable).  The source is smaller than the Infinity Cache, so repeated launches
                may read it from there: the rate is the kernel's, not a statement about HBM;
  host form     wall time, best of --host_repeats.

There is no pass mark: nothing earlier exists to regress against and nobody had measured this before, so this file records what
was measured and on what.  Prints one JSON line; --out writes it to a file (profiles/undistort_bench.json is one such run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uforecon_amd import colmap2mvsnet as M, ops, undistort as U  # noqa: E402

N, H, W, CHANNELS = 8, 1080, 1920, 3
# pincushion distortion: the output's corners look past the source picture at zoom 1, so `fit_zoom` runs its bisection
MODEL, PARAMS = "OPENCV", (1400.0, 1390.0, 962.3, 537.6, 0.10, -0.02, 0.001, -0.0005)
HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--host_repeats", type=int, default=2)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_undistort: no GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    raw = np.stack([np.stack([127 + 100 * np.sin(xx / (40.0 + 9 * c) + k) * np.cos(yy / (55.0 - 7 * c)) for c in range(CHANNELS)], -1)
                    for k in range(N)])
    raw = np.clip(raw + rng.normal(0, 4, raw.shape), 0, 255).astype(np.uint8)
    camera = M.Camera(1, MODEL, W, H, np.array(PARAMS))
    t0 = time.perf_counter()
    zoom = U.fit_zoom(MODEL, PARAMS, M.intrinsic_of(camera), H, W)
    fit_ms = (time.perf_counter() - t0) * 1e3
    Kz = U.zoomed(M.intrinsic_of(camera), zoom)
    k_out = (Kz[0, 0], Kz[1, 1], Kz[0, 2], Kz[1, 2])
    needed = 2 * N * H * W * CHANNELS + H * W
    res = dict(device=torch.cuda.get_device_name(0), workload=f"{N} x {H}x{W}x{CHANNELS} uint8, {MODEL} {list(PARAMS)}", zoom=zoom,
               fit_zoom_host_ms=fit_ms, repeats=a.repeats, bytes_needed=needed,
               timing="kernel: HIP events, mean over the repeats after a warm-up; call: host clock to a synchronise, per launch; "
                      "host form: wall, best of the host repeats", threshold=None,
               note="no threshold: nothing earlier exists to regress against; first measurement of this kernel")
    src = torch.from_numpy(raw).to(dev)
    dst, valid = ops.image_undistort_u8(src, MODEL, PARAMS, k_out, H, W)                  # warm: library, allocator, code object
    for _ in range(10):
        ops.image_undistort_u8(src, MODEL, PARAMS, k_out, H, W)
    torch.cuda.synchronize()
    ops.profile_enable(True)
    for _ in range(a.repeats):
        ops.image_undistort_u8(src, MODEL, PARAMS, k_out, H, W)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    res["kernel_ms"] = prof["image_undistort_u8"]["ms"] / a.repeats
    t0 = time.perf_counter()
    for _ in range(a.repeats):
        ops.image_undistort_u8(src, MODEL, PARAMS, k_out, H, W)
    torch.cuda.synchronize()
    res["call_ms"] = (time.perf_counter() - t0) * 1e3 / a.repeats
    res["achieved_TBs"] = needed / (res["kernel_ms"] * 1e-3) / 1e12
    res["hbm_peak_TBs"], res["hbm_achievable_TBs"] = HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS
    res["share_of_achievable_hbm"] = res["achieved_TBs"] / HBM_ACHIEVABLE_TBS
    times, want = [], None
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        want = U.undistort_host(raw, MODEL, PARAMS, k_out, H, W)
        times.append((time.perf_counter() - t0) * 1e3)
    res["host_form_ms"] = min(times)
    res["host_over_kernel"] = res["host_form_ms"] / res["kernel_ms"]
    res["equal_to_host_form"] = bool(np.array_equal(dst.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), want[1]))
    res["valid_share"] = float((want[1] == 255).mean())
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
