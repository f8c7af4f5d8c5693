"""Benchmark of the point-cloud filters (uforecon_amd/pcd_filter.py, csrc/points_filter.hip) on the 2 M-point sphere of
bench_render_points.py (radius 480 mm, seed 0) with a radial noise of 0.1 % of the radius added:
  * k-NN at k = 20 (every point's 20 nearest other points) and k = 30 (self included): the kernel alone (HIP events,
    ufr_profile_*) and ``ops.knn_points`` wall time, which adds the bounds, the keys, the two sorts and the un-permuting;
  * normals from the k = 30 rows, the voxel mean at 2 mm, and ``filter_points`` end to end (voxel, statistical, normals);
  * for scale only, the host: ``scipy.spatial.cKDTree(...).query(workers=16)`` for the two k-NN calls where scipy imports
    (distances compared), otherwise tests/pcd_ref.py on a stated subset; the numpy restatement of the normals (pcd_ref.py,
    numpy.linalg.eigh) on the whole cloud, and a bincount mean per voxel (another summation order: compared, not equal).
One run of every item (``runs`` in the result); nothing earlier exists to compare with, so no threshold is set.
Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pcd_ref as R  # noqa: E402
from bench_clean_mesh import VOXEL  # noqa: E402
from uforecon_amd import ops, pcd_filter  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def profiled(fn):
    ops.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    return {k: v["ms"] for k, v in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm, as bench_render_points")
    ap.add_argument("--noise", type=float, default=1e-3, help="radial noise as a share of the radius")
    ap.add_argument("--voxel_size", type=float, default=2.0)
    ap.add_argument("--subset", type=int, default=4000, help="queries of the pcd_ref fallback when scipy is absent")
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    d = rng.normal(size=(a.points, 3))
    radius = a.radius * VOXEL
    pts = d / np.linalg.norm(d, axis=1, keepdims=True) * radius
    pts = np.ascontiguousarray(pts * (1.0 + a.noise * rng.standard_normal(a.points))[:, None])
    colors = rng.integers(0, 256, (a.points, 3)).astype(np.uint8)
    p = torch.from_numpy(pts).cuda()
    c = torch.from_numpy(colors).cuda()
    ops.knn_points(p[:5000].contiguous(), p[:5000].contiguous(), 4)                        # warm: library, allocator
    res = dict(device=torch.cuda.get_device_name(0), runs=1,
               cloud=f"{a.points} points on a sphere of {radius} mm, radial noise {a.noise * radius} mm, uint8 colours")

    try:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        tree = cKDTree(pts)
        res["host_kdtree_build_ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError:
        tree = None
    for k, exclude_self in ((20, True), (30, False)):
        (idx, dist), wall = timed(lambda: ops.knn_points(p, p, k, exclude_self=exclude_self))
        item = dict(k=k, exclude_self=exclude_self, end_to_end_ms=wall,
                    kernel_ms=profiled(lambda: ops.knn_points(p, p, k, exclude_self=exclude_self))["points_knn"])
        if tree is not None:
            t0 = time.perf_counter()
            hd, hi = tree.query(pts, k + 1 if exclude_self else k, workers=16)
            item["host_kdtree_query_workers16_ms"] = (time.perf_counter() - t0) * 1e3
            hd = hd[:, 1:] if exclude_self else hd
            item["max_distance_difference_to_kdtree"] = float(np.abs(dist.cpu().numpy() - hd).max())
        else:
            sub = np.linspace(0, a.points - 1, a.subset).astype(np.int64)
            t0 = time.perf_counter()
            ri, rd = R.knn(pts[sub], pts, k + 1 if exclude_self else k)
            item["host_pcd_ref_ms"] = (time.perf_counter() - t0) * 1e3
            item["host_pcd_ref_queries"] = int(a.subset)
            ri = ri[:, 1:] if exclude_self else ri                  # the query itself comes first unless it has an exact duplicate
            item["subset_indices_equal_pcd_ref"] = bool(np.array_equal(idx.cpu().numpy()[sub], ri))
        res[f"knn_k{k}"] = item
    # normals from the k = 30 rows (still in idx)
    (nrm, curv, valid), wall = timed(lambda: ops.point_normals(p, idx))
    t0 = time.perf_counter()
    want_n, _, _, (_, w, _) = R.normals(pts, idx.cpu().numpy())
    host_ms = (time.perf_counter() - t0) * 1e3
    n_h = nrm.cpu().numpy()
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    angle = np.arctan2(np.linalg.norm(np.cross(n_h, want_n), axis=1), np.abs((n_h * want_n).sum(1)))
    res["normals_k30"] = dict(end_to_end_ms=wall, kernel_ms=profiled(lambda: ops.point_normals(p, idx))["points_normals"],
                              host_numpy_restatement_ms=host_ms, valid=int(valid.sum()), min_eigen_gap=float(gap.min()),
                              max_angle_to_eigh_rad_where_gap_above_1e3=float(angle[gap >= 1e-3].max()))
    # voxel mean
    (vp, vc, _, count), wall = timed(lambda: ops.voxel_downsample(p, a.voxel_size, c))
    prof = profiled(lambda: ops.voxel_downsample(p, a.voxel_size, c))
    t0 = time.perf_counter()
    keys = R.cell_keys(pts, pts.min(0) - a.voxel_size / 2, a.voxel_size)
    uniq, inv = np.unique(keys, return_inverse=True)
    cnt = np.bincount(inv)
    mean = np.stack([np.bincount(inv, pts[:, k]) / cnt for k in range(3)], 1)
    host_ms = (time.perf_counter() - t0) * 1e3
    res["voxel_mean"] = dict(voxel_size=a.voxel_size, voxels=int(len(vp)), end_to_end_ms=wall,
                             kernels_ms=prof["points_voxel_count"] + prof["points_voxel_mean"], host_bincount_ms=host_ms,
                             counts_equal_host=bool(np.array_equal(count.cpu().numpy(), cnt)),
                             max_position_difference_to_host=float(np.abs(vp.cpu().numpy() - mean).max()))
    # the whole filter
    out, wall = timed(lambda: pcd_filter.filter_points(p, c, voxel_size=a.voxel_size, nb_neighbors=20, std_ratio=2.0, normals_k=30))
    res["filter_points"] = dict(stages="voxel, statistical (20, 2.0), normals (30)", counts=out["counts"], end_to_end_ms=wall)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
