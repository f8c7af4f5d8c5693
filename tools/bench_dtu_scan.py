"""Benchmark of the DTU scan loader (uforecon_amd/dtu_scan.py, host_forms.py) at DTU's sizes: 3 views of 1600 x 1200 -> 800 x 640.
  * PNG decode on the host (PIL), per image;
  * the resize kernel (3 images in one launch) and the two ray calls, with HIP events (ufr_profile_*);
  * the same two steps in their host forms (numpy / CPU torch);
  * `DtuScan.__init__` plus one `scan[i]`, end to end, on the device and on the host.
The pictures are a smooth synthetic pattern with noise (random bytes alone would make the PNGs larger and slower to decode than
photographs).  There is no pass mark: these kernels are not the frame's hot path, and this file exists so that nobody has to
guess that.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uforecon_amd import cameras, host_forms as D, ops  # noqa: E402
from uforecon_amd.dtu_scan import DtuScan  # noqa: E402

ORIGINAL_WH, IMG_WH, VIEWS, SCAN = (1600, 1200), (800, 640), [23, 24, 33], "scan1"


def write_scan(root, rng):
    from PIL import Image

    os.makedirs(os.path.join(root, "cameras"))
    os.makedirs(os.path.join(root, SCAN, "image"))
    K = np.array([[2892.33, 0, 823.205], [0, 2883.175, 619.071], [0, 0, 1]])
    yy, xx = np.mgrid[0:ORIGINAL_WH[1], 0:ORIGINAL_WH[0]]
    for k, vid in enumerate(VIEWS):
        a = 0.3 * (k - 1)
        eye = 650.0 * np.array([np.sin(a), -np.cos(a) * np.cos(0.3), np.sin(0.3)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, -R @ eye
        rows = lambda m: [" ".join(repr(float(v)) for v in r) for r in m]  # noqa: E731
        with open(os.path.join(root, "cameras", "%08d_cam.txt" % vid), "w") as f:
            f.write("\n".join(["extrinsic"] + rows(E) + ["", "intrinsic"] + rows(K) + ["", "425.0 2.5", ""]))
        img = np.stack([127 + 100 * np.sin(xx / (40.0 + 9 * c) + k) * np.cos(yy / (55.0 - 7 * c)) for c in range(3)], -1)
        img = np.clip(img + rng.normal(0, 4, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, SCAN, "image", "%06d.png" % vid))


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
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = IMG_WH
    res = dict(views=len(VIEWS), original=f"{ORIGINAL_WH[1]}x{ORIGINAL_WH[0]}", image=f"{H}x{W}", device=torch.cuda.get_device_name(0),
               repeats=a.repeats, timing="best of the repeats; kernels by HIP events, mean over the repeats")
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "dtu_bench")
        write_scan(root, np.random.default_rng(0))
        paths = [os.path.join(root, SCAN, "image", "%06d.png" % v) for v in VIEWS]
        res["png_decode_ms_per_image"] = best_ms(lambda: [D.imread_rgb(p) for p in paths], a.repeats) / len(paths)
        raw = np.stack([D.imread_rgb(p) for p in paths])
        raw_dev = torch.from_numpy(raw).to(dev)
        scan = DtuScan(root, SCAN, img_wh=IMG_WH, original_img_wh=ORIGINAL_WH, test_view_pair=VIEWS, device=dev)   # warm: library, allocator
        batch = scan[0]
        m_ref, origin = batch["ref_pose_inv"][0].cpu().numpy(), batch["ray_o"][0].cpu().numpy()
        m_cam = np.eye(4, dtype=np.float32)       # any matrix costs the same
        torch.cuda.synchronize()
        ops.profile_enable(True)
        for _ in range(a.repeats):
            ops.image_resize_u8(raw_dev, H, W)
            ops.pixel_rays(m_ref, H, W, origin, dev)
            ops.pixel_rays(m_cam, H, W, None, dev)
        torch.cuda.synchronize()
        prof = ops.profile_read()
        ops.profile_enable(False)
        res["resize_kernel_ms"] = prof["image_resize_u8"]["ms"] / a.repeats
        res["ray_kernel_ms_per_call"] = prof["pixel_rays"]["ms"] / (2 * a.repeats)
        res["upload_ms"] = best_ms(lambda: (torch.from_numpy(raw).to(dev), torch.cuda.synchronize()), a.repeats)
        res["host_resize_ms"] = best_ms(lambda: D.image_planes_host(raw, H, W), a.repeats)
        hp = cameras.homo_pixels(H, W)
        res["host_rays_ms_per_call"] = best_ms(lambda: (D.pixel_rays_host(m_ref, H, W, origin, hp), D.pixel_rays_host(m_cam, H, W, None, hp)),
                                               a.repeats) / 2

        def end_to_end(device):
            s = DtuScan(root, SCAN, img_wh=IMG_WH, original_img_wh=ORIGINAL_WH, test_view_pair=VIEWS, device=device)
            s[0]
            if device != "cpu":
                torch.cuda.synchronize()

        res["scan_and_first_batch_ms_device"] = best_ms(lambda: end_to_end(dev), a.repeats)
        res["scan_and_first_batch_ms_host"] = best_ms(lambda: end_to_end("cpu"), a.repeats)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
