"""What tests/test_dtu_scan.py and tests/test_gpu_dtu_scan.py share: tests/golden/dtu_scan_small.npz (written by
tests/golden/make_golden_dtu_scan.py) read once, and the scan directory rebuilt from it."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RAY_KEYS = ("ray_d", "cam_ray_d")
IMAGE_KEYS = ("ref_img", "source_imgs")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(HERE, "golden", "dtu_scan_small.npz"))
    return {k: z[k] for k in z.files}


def cases():
    return json.loads(str(golden()["cases"]))


def write_scan(tmp_path):
    """<tmp>/<root name>/cameras/%08d_cam.txt and <scan>/image/%06d.png, as the generator wrote them; returns (root, scan)."""
    from PIL import Image

    g = golden()
    root, scan = os.path.join(str(tmp_path), str(g["root_name"])), str(g["scan"])
    os.makedirs(os.path.join(root, "cameras"), exist_ok=True)
    os.makedirs(os.path.join(root, scan, "image"), exist_ok=True)
    for k in g:
        if k.startswith("cam/"):
            with open(os.path.join(root, "cameras", "%08d_cam.txt" % int(k[4:])), "w") as f:
                f.write(str(g[k]))
        elif k.startswith("img/"):
            Image.fromarray(g[k]).save(os.path.join(root, scan, "image", "%06d.png" % int(k[4:])))
    return root, scan


def open_scan(root, scan, case, device):
    from uforecon_amd.dtu_scan import DtuScan

    return DtuScan(root, scan, original_img_wh=[int(v) for v in golden()["original_img_wh"]], device=device, **cases()[case])


def golden_batch(case, i):
    """{key: array} of render view ``i``; proj_matrices as `proj_matrices.stageN`, meta as a str"""
    pre = f"{case}/{i}/"
    return {k[len(pre):]: (str(v) if k.endswith("/meta") else v) for k, v in golden().items() if k.startswith(pre)}


def flat_batch(batch):
    """a loader batch in the same flat form, tensors as numpy arrays"""
    out = {}
    for k, v in batch.items():
        if k == "proj_matrices":
            out.update({f"proj_matrices.{st}": t.cpu().numpy() for st, t in v.items()})
        elif k == "meta":
            assert isinstance(v, list) and len(v) == 1
            out[k] = v[0]
        else:
            out[k] = v.cpu().numpy()
    return out


def ulps_of_scale(got, want):
    """largest |got - want| in float32 steps at the key's largest magnitude: the measure of DESIGN 3.4.4 for entries that went
    through another machine's LAPACK / BLAS (an entry near zero is a difference of large ones: its own ulp would say nothing)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max() / np.spacing(np.float32(scale))) if scale > 0 else float(np.abs(got).max() > 0)


# Bounds, in `ulps_of_scale`, for the entries of a batch that come out of LAPACK / BLAS calls (inverses, the QR of the
# decomposition, 4x4 products).  On the machine that wrote the golden file every entry is equal bit for bit; the figures are
# the largest departures measured on a second machine (another CPU, so other kernels of the same libraries), times four
# (DESIGN 3.4.4).  A key that is not listed came out equal there as well and is tested for equality.
TOL_ULPS = {"scale_mat": 4, "ref_pose": 6, "w2cs": 8, "near_fars": 8, "scale_factor": 8, "source_poses": 8, "ref_pose_inv": 8,
            "source_poses_inv": 8, "ray_o": 8, "ray_d": 8}      # measured: 1, 1.5, and 2 for the rest


def assert_matches_golden(got, want, what, ray_atol=0.0):
    """a flat batch against a golden one: same keys, shapes, dtypes, meta; values equal, or within TOL_ULPS where listed; the ray
    tables additionally get ``ray_atol`` (the device kernel's bound against the host form)"""
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        if k == "meta":
            assert got[k] == w, (what, got[k], w)
            continue
        assert got[k].shape == w.shape and got[k].dtype == w.dtype, (what, k, got[k].shape, got[k].dtype)
        if k in TOL_ULPS or (k in RAY_KEYS and ray_atol > 0):
            step = np.spacing(np.float32(np.abs(w).max()))
            bound = TOL_ULPS.get(k, 0.0) * float(step) + (ray_atol if k in RAY_KEYS else 0.0)
            worst = float(np.abs(got[k].astype(np.float64) - w).max())
            assert worst <= bound, (what, k, worst, bound, ulps_of_scale(got[k], w))
        else:
            assert np.array_equal(got[k], w), (what, k, ulps_of_scale(got[k], w))


def to_device(batch, device):
    """a loader batch moved to ``device`` (meta and the proj_matrices dict kept)"""
    import torch

    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
    out["proj_matrices"] = {st: t.to(device) for st, t in batch["proj_matrices"].items()}
    return out
