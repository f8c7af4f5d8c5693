"""Poisson surface reconstruction on the GPU: from an oriented point cloud to a mesh.

The step that closes the point route (``depth_fusion`` -> ``pcd_filter --normals`` -> here), which the reference leaves to
Open3D's ``create_from_point_cloud_poisson``::

    python -m uforecon_amd.poisson_mesh --root_dir OUT_F --out_dir OUT_P --resolution 256 --min_density 0.5 --color

reads ``OUT_F/pcd/scan<N>.ply`` (x y z, nx ny nz and optionally red green blue, what ``pcd_filter --normals`` writes) and
writes ``OUT_P/mesh/scan<N>.ply`` and ``OUT_P/poisson_mesh.json`` (the grid, the iso value and the solver's report per
scan); ``clean_mesh``, ``dtu_eval --mesh_dir OUT_P/mesh`` and ``render_trajectory --mesh_dir OUT_P/mesh`` read the meshes
as they stand.  The rules are stated in include/ufr.h ("Poisson surface reconstruction") and restated in numpy / scipy in
tests/poisson_ref.py: a UNIFORM grid (no adaptive octree), no screening term, plain conjugate gradients (no multigrid).

  grid        h = the largest extent of the samples / ``resolution``; ``pad`` cells of margin on every side.
  splat       V = sum of w n and W = sum of w with the trilinear weights w of every sample on the 8 nodes of its cell.
  divergence  b = div V by central differences.
  solve       A chi = -b, A = the negated 7-point Laplacian with chi = 0 outside the grid (csrc/poisson.hip).
  surface     iso = the mean of chi at the samples; marching cubes on chi - iso; density = W at every vertex;
              ``min_density`` > 0 drops the vertices below it and every face that touches one.

With normals that point outwards chi rises outwards, so faces and normals come out as for a TSDF.  ``min_density`` = 0
keeps the watertight surface, which closes itself far from the samples where the cloud is partial; that closure is what
``min_density`` or ``clean_mesh`` removes.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys

import numpy as np


def _cuda64(a, name):
    import torch

    from .ops import UfrError

    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, np.float64).reshape(-1, 3)).cuda()
    if a.dim() != 2 or a.shape[1] != 3:
        raise UfrError(f"{name}: expected shape (N, 3), got {tuple(a.shape)}")
    return a.to(torch.float64).contiguous()


def trim_mesh(verts, faces, normals, density, min_density):
    """Drops the vertices with ``density < min_density`` and every face that touches one; indices are compacted and the
    order of the kept vertices and faces is preserved.  Returns ``(verts, faces, normals, density, keep)``, ``keep`` the
    mask over the input vertices."""
    import torch

    keep = density >= float(min_density)
    fkeep = keep[faces.long()].all(1) if faces.shape[0] else torch.zeros(0, dtype=torch.bool, device=faces.device)
    remap = (torch.cumsum(keep.to(torch.int64), 0) - 1).to(torch.int32)
    return verts[keep], remap[faces[fkeep].long()].contiguous(), normals[keep], density[keep], keep


def reconstruct(points, normals, colors=None, resolution=256, pad=4, tol=1e-6, max_iter=None, min_density=0.0, check_every=16):
    """``(verts (V,3) float64, faces (F,3) int32, normals (V,3) float32, density (V,) float64, colors (V,3) uint8 or None,
    info)`` of the samples ``points`` (N,3) with unit ``normals`` (N,3) and optional ``colors`` (N,3) uint8: numpy arrays or
    CUDA tensors in, CUDA tensors out, vertices in scene coordinates.  Samples whose normal is not finite or is 0 are
    dropped and counted (``info['dropped']``).  ``info`` also carries ``dims``, ``h``, ``origin``, ``iso``, ``iterations``,
    ``residual`` and ``converged``; a solve that reaches ``max_iter`` (default 8 max(dims)) is reported there, not raised.
    Raises UfrError for resolution < 4, pad < 2, a grid of 2^31 nodes or more, a cloud without extent or with coordinates
    that are not finite, and a cloud without a usable normal."""
    import torch

    from . import ops
    from .ops import UfrError

    points, normals = _cuda64(points, "points"), _cuda64(normals, "normals")
    if normals.shape != points.shape:
        raise UfrError(f"normals: expected shape {tuple(points.shape)}, got {tuple(normals.shape)}")
    if colors is not None:
        if not isinstance(colors, torch.Tensor):
            colors = torch.from_numpy(np.ascontiguousarray(colors, np.uint8).reshape(-1, 3))
        colors = colors.to(points.device)
        if tuple(colors.shape) != tuple(points.shape) or colors.dtype != torch.uint8:
            raise UfrError(f"colors: expected uint8 of shape {tuple(points.shape)}")
    ok = torch.isfinite(normals).all(1) & ((normals * normals).sum(1) > 0.0)
    dropped = int(points.shape[0] - int(ok.sum()))
    if dropped:
        points, normals = points[ok].contiguous(), normals[ok].contiguous()
        colors = None if colors is None else colors[ok].contiguous()
    if points.shape[0] == 0:
        raise UfrError("reconstruct: no sample with a finite, non-zero normal")
    origin, h, dims = ops.poisson_grid(points, resolution, pad)
    V, W = ops.poisson_splat(points, normals, origin, h, dims)
    b = ops.poisson_divergence(V, h)
    del V
    chi, info = ops.poisson_solve(b, h, tol, max_iter, check_every)
    del b
    _, iso = ops.poisson_sample(chi, origin, h, points, return_mean=True)
    iso = float(iso)
    v, faces, vn = ops.marching_cubes((chi - iso).float(), 0.0)
    verts = torch.tensor(origin, dtype=torch.float64, device=points.device) + h * v.to(torch.float64)
    density = ops.poisson_sample(W, origin, h, verts.contiguous())
    if min_density > 0.0:
        verts, faces, vn, density, _ = trim_mesh(verts, faces, vn, density, min_density)
    verts = verts.contiguous()
    vcol = None
    if colors is not None:
        vcol = torch.zeros((verts.shape[0], 3), dtype=torch.uint8, device=points.device)
        if verts.shape[0]:
            idx, _ = ops.knn_points(verts, points, 1)
            vcol = colors[idx[:, 0].long()].contiguous()
    info = dict(dims=list(dims), h=h, origin=list(origin), iso=iso, iterations=info["iterations"], residual=info["residual"],
                converged=info["converged"], dropped=dropped)
    return verts, faces, vn.contiguous(), density.contiguous(), vcol, info


# ------------------------------------------------------------------ files
class NoNormals(ValueError):
    pass


def reconstruct_file(src, dst, normals_k=0, viewpoints=None, color=False, **params):
    """``reconstruct`` from a PLY cloud to a PLY mesh (tsdf.meshwrite's layout); returns ``info`` with the mesh's counts.  A
    cloud without nx ny nz raises NoNormals unless ``normals_k`` > 0 estimates them (pcd_filter.estimate_normals)."""
    from .dtu_eval import read_ply
    from .tsdf import meshwrite

    xyz, _, rgb, nrm = read_ply(src, with_colors=True, with_normals=True)
    if nrm is None:
        if not normals_k:
            raise NoNormals(src)
        from .pcd_filter import estimate_normals

        nrm, _, _ = estimate_normals(xyz, normals_k, viewpoints)      # points without a normal get zeros and are dropped
    verts, faces, vn, density, vcol, info = reconstruct(xyz, nrm, rgb if color else None, **params)
    V = int(verts.shape[0])
    col = vcol.cpu().numpy() if vcol is not None else np.full((V, 3), 255, np.uint8)
    meshwrite(dst, verts.cpu().numpy(), faces.cpu().numpy(), vn.cpu().numpy(), col)
    return dict(info, samples=int(len(xyz)), vertices=V, faces=int(faces.shape[0]))


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--root_dir", type=str, default="./outputs", help="reads <root_dir>/pcd/scan<N>.ply")
    parser.add_argument("--out_dir", type=str, required=True, help="writes <out_dir>/mesh/*.ply and <out_dir>/poisson_mesh.json")
    parser.add_argument("--scans", type=int, nargs="+", default=None, help="scan numbers (default: every pcd/scan*.ply found)")
    parser.add_argument("--ply", type=str, nargs="+", default=None, help="named files instead, written to <out_dir>/mesh/<stem>.ply")
    parser.add_argument("--resolution", type=int, default=256, help="cells along the largest extent of the samples (>= 4)")
    parser.add_argument("--pad", type=int, default=4, help="cells of margin on every side (>= 2)")
    parser.add_argument("--tol", type=float, default=1e-6, help="the solve ends at |r| <= tol |b|")
    parser.add_argument("--max_iter", type=int, default=None, help="most iterations (default: 8 x the largest grid dimension)")
    parser.add_argument("--min_density", type=float, default=0.0, help="drop vertices whose sample density is below this; 0: watertight")
    parser.add_argument("--color", action="store_true", help="give every vertex the colour of its nearest sample")
    parser.add_argument("--normals", type=int, default=0, metavar="K", help="estimate missing normals from K neighbours (3 .. 32)")
    parser.add_argument("--dataset_dir", type=str, default=None, help="dataset (cameras/<view>_cam.txt) estimated normals face")
    parser.add_argument("--views", type=int, nargs="+", default=[23, 24, 33], help="the views whose camera centres they face")
    return parser


def main(argv=None) -> int:
    from .pcd_filter import KNN_MAX_K, camera_centres

    args = make_parser().parse_args(argv)
    if args.normals and not 3 <= args.normals <= KNN_MAX_K:
        print("poisson_mesh: --normals {} (must be 3 .. {})".format(args.normals, KNN_MAX_K))
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
            print("poisson_mesh: no --dataset_dir: estimated normals are oriented by their largest component, not towards a camera")
    os.makedirs(os.path.join(args.out_dir, "mesh"), exist_ok=True)
    params = dict(resolution=args.resolution, pad=args.pad, tol=args.tol, max_iter=args.max_iter, min_density=args.min_density)
    report = dict(params=dict(params, color=args.color, normals=args.normals), scans={})
    for name, src in jobs:
        if not os.path.exists(src):
            print("cloud not found: {}".format(src))
            continue
        try:
            info = reconstruct_file(src, os.path.join(args.out_dir, "mesh", name + ".ply"), args.normals, viewpoints, args.color, **params)
        except NoNormals:
            print("poisson_mesh: {} has no normals (nx ny nz): write them with pcd_filter --normals K, or pass --normals K here".format(src))
            return 1
        report["scans"][name] = info
        print(name, "{} samples -> {} vertices, {} faces; grid {}, {} iterations, residual {:.3g}{}".format(
            info["samples"], info["vertices"], info["faces"], "x".join(str(d) for d in info["dims"]), info["iterations"],
            info["residual"], "" if info["converged"] else " (NOT converged)"))
    with open(os.path.join(args.out_dir, "poisson_mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
