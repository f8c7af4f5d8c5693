"""Point-cloud filtering on the GPU: voxel downsampling, statistical and radius outlier removal, normal estimation.

The cleanup an MVS pipeline runs between depth fusion and scoring, which the reference leaves to Open3D::

    python -m uforecon_amd.pcd_filter --root_dir OUT --out_dir OUT_F --voxel_size 0.5 --nb_neighbors 20 --std_ratio 2 \\
        --normals 30 --dataset_dir DTU_TEST --views 23 24 33

reads ``OUT/pcd/scan<N>.ply`` (what ``depth_fusion`` writes) and writes ``OUT_F/pcd/scan<N>.ply`` and ``OUT_F/pcd_filter.json``
(the counts after every stage, per scan); ``dtu_eval --outdir OUT_F --mode pcd`` and ``render_trajectory --pcd_dir OUT_F/pcd``
read the result as they read the input.  The stages run in the order voxel, statistical, radius, normals; a stage whose
parameter is 0 is skipped.  They rest on ``ops.knn_points`` / ``ops.voxel_downsample`` / ``ops.point_normals``
(csrc/points_filter.hip); the rules are stated in include/ufr.h ("point-cloud filtering") and restated in numpy in
tests/pcd_ref.py.  They follow the public descriptions of PCL's StatisticalOutlierRemoval / RadiusOutlierRemoval / VoxelGrid
and Open3D's equivalents; neither library was compared against.

  statistical   avg_i = the mean distance from point i to its ``nb_neighbors`` nearest other points; a point is kept iff
                avg_i <= mean(avg) + std_ratio * std(avg) (population standard deviation over the finite avg).
  radius        a point is kept iff at least ``nb_points`` other points lie within ``radius`` (inclusive).
  voxel         one point per occupied voxel: mean position, rounded mean colour, renormalised normal sum.
  normals       the eigenvector of the smallest eigenvalue of the covariance of the ``k`` nearest points (the point itself
                included), turned towards the camera centre that sees it most squarely, or, without cameras, so that its
                largest component is positive.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys

import numpy as np

KNN_MAX_K = 32


def _points(points):
    import torch

    if isinstance(points, torch.Tensor):
        return points
    return torch.from_numpy(np.ascontiguousarray(points, np.float64).reshape(-1, 3)).cuda()


def remove_statistical_outliers(points, nb_neighbors=20, std_ratio=2.0):
    """``(keep, avg, threshold)`` of a cloud ((N,3) CUDA float64, or a numpy array that is copied to the GPU): ``avg`` (N,)
    float64 = the mean distance to the ``nb_neighbors`` (1 .. 32) nearest other points, the left-to-right sum over the slots
    the k-NN filled divided by their number, inf for a point with no other point; ``threshold`` = mean + ``std_ratio`` *
    population standard deviation over the finite ``avg`` (a float); ``keep`` (N,) bool = ``avg <= threshold``."""
    import torch

    from . import ops

    points = _points(points)
    N = int(points.shape[0])
    if N == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device), torch.zeros(0, dtype=torch.float64, device=points.device), float("inf")
    idx, dist = ops.knn_points(points, points, nb_neighbors, exclude_self=True)
    filled = idx >= 0
    s = torch.zeros(N, dtype=torch.float64, device=points.device)
    for j in range(idx.shape[1]):                     # slot by slot: the order the rule states
        s = s + torch.where(filled[:, j], dist[:, j], torch.zeros_like(s))
    m = filled.sum(1)
    avg = torch.where(m > 0, s / m.clamp(min=1).to(torch.float64), torch.full_like(s, float("inf")))
    fin = avg[torch.isfinite(avg)]
    threshold = float(fin.mean() + float(std_ratio) * fin.std(unbiased=False)) if fin.numel() else float("inf")
    return avg <= threshold, avg, threshold


def remove_radius_outliers(points, nb_points, radius):
    """``keep`` (N,) bool: at least ``nb_points`` (1 .. 32) other points lie within ``radius`` (inclusive)."""
    import torch

    from . import ops

    points = _points(points)
    if int(points.shape[0]) == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    idx, _ = ops.knn_points(points, points, nb_points, max_dist=radius, exclude_self=True)
    return (idx >= 0).sum(1) >= int(nb_points)


def estimate_normals(points, k=30, viewpoints=None):
    """``(normals (N,3) float64, curvature (N,) float64, valid (N,) uint8)`` from every point's ``k`` (1 .. 32) nearest
    points, itself included; ``viewpoints`` (V,3): the camera centres the normals are turned towards (None: the largest
    component is made positive).  A point with fewer than three neighbours gets valid 0 and zeros."""
    import torch

    from . import ops

    points = _points(points)
    if int(points.shape[0]) == 0:
        z = torch.zeros((0, 3), dtype=torch.float64, device=points.device)
        return z, z[:, 0].clone(), torch.zeros(0, dtype=torch.uint8, device=points.device)
    idx, _ = ops.knn_points(points, points, k)
    return ops.point_normals(points, idx, None if viewpoints is None else _points(viewpoints))


def filter_points(points, colors=None, voxel_size=0, nb_neighbors=20, std_ratio=2.0, radius=0, nb_points=0, normals_k=0,
                  viewpoints=None):
    """Voxel downsampling, then the statistical filter, then the radius filter, then normals; ``voxel_size`` 0, ``nb_neighbors``
    0, ``radius`` or ``nb_points`` 0 and ``normals_k`` 0 skip their stage.  ``points`` (N,3) and ``colors`` (N,3) uint8 or None:
    numpy arrays or CUDA tensors.  Returns a dict of CUDA tensors ``points``, ``colors`` / ``normals`` / ``curvature`` / ``valid``
    (None where absent), and ``counts``: the number of points at the input and after every stage that ran."""
    import torch

    from . import ops

    points = _points(points).contiguous()
    if colors is not None and not isinstance(colors, torch.Tensor):
        colors = torch.from_numpy(np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)).cuda()
    counts = dict(input=int(points.shape[0]))
    if voxel_size and points.shape[0]:
        points, colors, _, _ = ops.voxel_downsample(points, voxel_size, colors)
        counts["voxel"] = int(points.shape[0])
    for name, on in (("statistical", nb_neighbors), ("radius", radius and nb_points)):
        if not on or not points.shape[0]:
            continue
        keep = (remove_statistical_outliers(points, nb_neighbors, std_ratio)[0] if name == "statistical"
                else remove_radius_outliers(points, nb_points, radius))
        points = points[keep].contiguous()
        colors = None if colors is None else colors[keep].contiguous()
        counts[name] = int(points.shape[0])
    normals = curvature = valid = None
    if normals_k:
        normals, curvature, valid = estimate_normals(points, normals_k, viewpoints)
        counts["normals_valid"] = int(valid.sum())
    return dict(points=points, colors=colors, normals=normals, curvature=curvature, valid=valid, counts=counts)


# ------------------------------------------------------------------ files
def write_ply(filename, xyz, rgb=None, normals=None):
    """A binary little-endian PLY: x y z (float), red green blue (uchar) when given, nx ny nz (float) when given."""
    fields = [(n, "<f4") for n in "xyz"]
    fields += [(n, "u1") for n in ("red", "green", "blue")] if rgb is not None else []
    fields += [(n, "<f4") for n in ("nx", "ny", "nz")] if normals is not None else []
    rec = np.empty(len(xyz), dtype=fields)
    for names, arr in ((("x", "y", "z"), xyz), (("red", "green", "blue"), rgb), (("nx", "ny", "nz"), normals)):
        if arr is not None:
            for k, name in enumerate(names):
                rec[name] = np.asarray(arr)[:, k]
    kinds = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(rec)
    header += "".join("property %s %s\n" % (kinds[t], n) for n, t in fields) + "end_header\n"
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def camera_centres(dataset_dir, views):
    """(V,3) float64: the centres of ``<dataset_dir>/cameras/<view>_cam.txt``, -R^T t of the world-to-camera matrix."""
    from .cameras import read_cam_file

    out = []
    for v in views:
        _, E, _ = read_cam_file(os.path.join(dataset_dir, "cameras/{:0>8}_cam.txt".format(v)))
        E = E.astype(np.float64)
        out.append(-E[:3, :3].T @ E[:3, 3])
    return np.array(out, np.float64).reshape(-1, 3)


def filter_file(src, dst, viewpoints=None, **params):
    """``filter_points`` from one PLY file to another; returns the counts."""
    from .dtu_eval import read_ply

    xyz, _, rgb = read_ply(src, with_colors=True)
    out = filter_points(xyz, rgb, viewpoints=viewpoints, **params)
    host = {k: None if out[k] is None else out[k].cpu().numpy() for k in ("points", "colors", "normals")}
    write_ply(dst, host["points"], host["colors"], host["normals"])
    return out["counts"]


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--root_dir", type=str, default="./outputs", help="reads <root_dir>/pcd/scan<N>.ply")
    parser.add_argument("--out_dir", type=str, required=True, help="writes <out_dir>/pcd/*.ply and <out_dir>/pcd_filter.json")
    parser.add_argument("--scans", type=int, nargs="+", default=None, help="scan numbers (default: every pcd/scan*.ply found)")
    parser.add_argument("--ply", type=str, nargs="+", default=None, help="named files instead, written to <out_dir>/pcd/<stem>.ply")
    parser.add_argument("--voxel_size", type=float, default=0.0, help="voxel edge; 0: no downsampling")
    parser.add_argument("--nb_neighbors", type=int, default=20, help="neighbours of the statistical filter (1 .. 32); 0: skip it")
    parser.add_argument("--std_ratio", type=float, default=2.0, help="standard deviations above the mean that are kept")
    parser.add_argument("--radius", type=float, default=0.0, help="radius of the radius filter; 0: skip it")
    parser.add_argument("--nb_points", type=int, default=0, help="points required within --radius (1 .. 32); 0: skip it")
    parser.add_argument("--normals", type=int, default=0, metavar="K", help="estimate normals from K neighbours (3 .. 32); 0: none")
    parser.add_argument("--dataset_dir", type=str, default=None, help="dataset (cameras/<view>_cam.txt) the normals face")
    parser.add_argument("--views", type=int, nargs="+", default=[23, 24, 33], help="the views whose camera centres the normals face")
    return parser


def main(argv=None) -> int:
    args = make_parser().parse_args(argv)
    if os.path.abspath(args.out_dir) == os.path.abspath(args.root_dir):
        print("pcd_filter: --out_dir equals --root_dir ({}): the filtered clouds would overwrite their input".format(args.root_dir))
        return 2
    for name, k in (("--nb_neighbors", args.nb_neighbors), ("--nb_points", args.nb_points), ("--normals", args.normals)):
        if not 0 <= k <= KNN_MAX_K:
            print("pcd_filter: {} {} (must be 0 .. {})".format(name, k, KNN_MAX_K))
            return 2
    if args.normals in (1, 2):
        print("pcd_filter: --normals {} (a normal needs at least 3 neighbours; 0 skips the stage)".format(args.normals))
        return 2
    if args.ply:
        jobs = [(os.path.splitext(os.path.basename(p))[0], p) for p in args.ply]
    elif args.scans:
        jobs = [("scan{}".format(s), os.path.join(args.root_dir, "pcd", "scan{}.ply".format(s))) for s in args.scans]
    else:
        found = sorted(glob.glob(os.path.join(args.root_dir, "pcd", "scan*.ply")))
        jobs = [(os.path.splitext(os.path.basename(p))[0], p) for p in found]
    viewpoints = None
    if args.normals:
        if args.dataset_dir:
            viewpoints = camera_centres(args.dataset_dir, args.views)
        else:
            print("pcd_filter: no --dataset_dir: normals are oriented by their largest component, not towards a camera")
    os.makedirs(os.path.join(args.out_dir, "pcd"), exist_ok=True)
    params = dict(voxel_size=args.voxel_size, nb_neighbors=args.nb_neighbors, std_ratio=args.std_ratio, radius=args.radius,
                  nb_points=args.nb_points, normals_k=args.normals)
    report = dict(params=dict(params, views=list(args.views) if viewpoints is not None else None), scans={})
    for name, src in jobs:
        if not os.path.exists(src):
            print("cloud not found: {}".format(src))
            continue
        dst = os.path.join(args.out_dir, "pcd", name + ".ply")
        counts = filter_file(src, dst, viewpoints, **params)
        report["scans"][name] = counts
        print(name, " -> ".join("{} {}".format(k, v) for k, v in counts.items()))
    with open(os.path.join(args.out_dir, "pcd_filter.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
