"""Mesh smoothing on the GPU: Taubin and Laplacian steps with cotangent or uniform weights -- the denoising stage of the mesh
route, between ``clean_mesh`` and ``simplify_mesh``; the reference leaves it to Open3D and trimesh.  Every kernel is in
csrc/mesh_smooth.hip (through ``ops.mesh_smooth``); include/ufr.h states every rule, tests/smooth_ref.py restates them in numpy.

    python -m uforecon_amd.smooth_mesh --mesh_dir OUT/mesh/final --out_dir OUT/mesh/smooth [--method taubin|laplacian]
        [--weights cotangent|uniform] [--iterations 10] [--lam 0.5] [--mu M] [--boundary fixed|free] [--scans ...] [--ply FILE ...]

reads ``<mesh_dir>/scan<N>.ply`` (with its vertex colours when it has them), writes ``<out_dir>/scan<N>.ply`` and
``<out_dir>/smooth_mesh.json`` with the counts, the displacement and the enclosed volume of every scan.  ``--ply`` smooths the
named mesh files instead, each to ``<out_dir>/<file stem>.ply``.  Only the vertex positions change: faces, vertex order and
colours pass through, so the output goes as it stands through ``simplify_mesh``, ``color_mesh``, ``dtu_eval`` and
``render_trajectory``.

1. the corner slots are sorted by vertex once (stable): a vertex's rows are its incident corners in ascending slot;
2. a row weighs the face's two other corners by 1 (``uniform``) or by the cotangents of the angles opposite, taken from the
   input positions and clamped to 0 .. 64 (``cotangent``); a face that names a vertex twice, or has no area, contributes nothing;
3. one step moves a vertex by ``t`` times the weighted mean of its neighbours' offsets, every read from the previous positions;
   ``laplacian`` takes ``iterations`` steps with ``lam``, ``taubin`` alternates ``lam`` and ``mu`` (default ``1 / (0.1 - 1 / lam)``)
   and does not shrink the surface;
4. a border vertex -- some neighbour does not occur exactly twice -- stays where it is unless ``--boundary free``.

An edge is rounded like noise here: the feature-preserving filter is ``denoise_mesh``.  Open3D's ``filter_smooth_taubin`` and
``filter_smooth_laplacian`` were not compared against, and no real scan has been smoothed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from .dtu_eval import DTU_SCANS, read_ply


def smooth_mesh(verts, faces, method="taubin", weights="cotangent", iterations=10, lam=0.5, mu=None, boundary="fixed", pinned=None,
                device="cuda"):
    """A mesh smoothed in memory.  ``verts`` (V,3) any float dtype (widened to float64 once), ``faces`` (F,3) integers,
    ``pinned`` (V,) uint8 or None; the other arguments are those of ``ops.mesh_smooth``.  Returns its dict with numpy arrays:
    ``verts`` (V,3) float64 and ``border`` (V,) uint8."""
    import torch

    from . import ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if len(faces) and (faces.min() < -2 ** 31 or faces.max() >= 2 ** 31):
        raise UfrError(f"smooth_mesh: face indices span {faces.min()}..{faces.max()}")
    dev = torch.device(device)
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)
    tp = None
    if pinned is not None:
        pinned = np.asarray(pinned)
        if pinned.dtype != np.uint8:
            raise UfrError(f"smooth_mesh: pinned {pinned.dtype}: expected uint8")
        tp = torch.from_numpy(np.ascontiguousarray(pinned)).to(dev)
    out = ops.mesh_smooth(tv, tf, method=method, weights=weights, iterations=iterations, lam=lam, mu=mu, boundary=boundary, pinned=tp)
    return {k: v.cpu().numpy() for k, v in out.items()}


def signed_volume(verts, faces):
    """the volume a mesh encloses (the sum of its faces' signed tetrahedra with the origin), float64 on the host"""
    a, b, c = (np.asarray(verts, np.float64)[np.asarray(faces)[:, e]] for e in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh_dir", type=str, default="./outputs/mesh/final", help="directory of scan<N>.ply")
    parser.add_argument("--out_dir", type=str, default="./outputs/mesh/smooth", help="scan<N>.ply and smooth_mesh.json go here")
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    parser.add_argument("--ply", type=str, nargs="+", default=None,
                        help="smooth these mesh files instead of scan<N>.ply, each to <out_dir>/<file stem>.ply")
    parser.add_argument("--method", choices=["taubin", "laplacian"], default="taubin",
                        help="taubin: a lam step then a mu step per iteration (no shrinkage); laplacian: one lam step")
    parser.add_argument("--weights", choices=["cotangent", "uniform"], default="cotangent",
                        help="cotangent: from the input's angles, clamped to 0 .. 64; uniform: every neighbour weighs 1")
    parser.add_argument("--iterations", type=int, default=10)
    parser.add_argument("--lam", type=float, default=0.5, help="the step factor, in (0, 1]")
    parser.add_argument("--mu", type=float, default=None, help="taubin's second factor, below -lam (default: 1 / (0.1 - 1 / lam))")
    parser.add_argument("--boundary", choices=["fixed", "free"], default="fixed", help="fixed: border vertices stay where they are")
    return parser


def smooth_file(mesh_path, out_path, method="taubin", weights="cotangent", iterations=10, lam=0.5, mu=None, boundary="fixed",
                device="cuda"):
    """One mesh file: reads ``mesh_path``, writes ``out_path`` (with colours when the input has them).  Returns the report
    dict of ``smooth_mesh.json``.  Raises ValueError with one line for a mesh without faces."""
    from . import ops
    from .clean_mesh import write_ply
    from .color_mesh import write_ply as write_ply_colors

    verts, faces, colors = read_ply(mesh_path, with_colors=True)
    if faces is None or len(faces) == 0:
        raise ValueError(f"{mesh_path} has no faces")
    r = smooth_mesh(verts, faces, method=method, weights=weights, iterations=iterations, lam=lam, mu=mu, boundary=boundary,
                    device=device)
    if colors is not None:
        write_ply_colors(out_path, r["verts"], faces, colors)
    else:
        write_ply(out_path, r["verts"], faces)
    moved = np.linalg.norm(r["verts"] - np.asarray(verts, np.float64), axis=1)
    factors = ops.smooth_factors(method, iterations, lam, mu)
    return dict(mesh=mesh_path, method=method, weights=weights, iterations=int(iterations), lam=float(lam),
                mu=float(factors[1]) if method == "taubin" and factors else None, boundary=boundary, vertices=int(len(verts)),
                faces=int(len(faces)), border_vertices=int(r["border"].sum()), mean_displacement=float(moved.mean()),
                max_displacement=float(moved.max()), volume_in=signed_volume(verts, faces),
                volume_out=signed_volume(r["verts"], faces), colors=colors is not None)


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.iterations < 0:
        parser.error(f"--iterations {args.iterations}: must be >= 0")
    if not 0.0 < args.lam <= 1.0:
        parser.error(f"--lam {args.lam}: must be in (0, 1]")
    if args.mu is not None and not args.mu < -args.lam:
        parser.error(f"--mu {args.mu}: must be below -lam = {-args.lam}")
    if args.ply is not None:
        jobs = [(os.path.splitext(os.path.basename(p))[0], p) for p in args.ply]
    else:
        jobs = [("scan%d" % scan, os.path.join(args.mesh_dir, "scan%d.ply" % scan)) for scan in args.scans]
    os.makedirs(args.out_dir, exist_ok=True)
    report = {}
    for name, path in jobs:
        if not os.path.exists(path):
            print("%s: no mesh at %s" % (name, path))
            continue
        try:
            report[name] = smooth_file(path, os.path.join(args.out_dir, name + ".ply"), method=args.method, weights=args.weights,
                                       iterations=args.iterations, lam=args.lam, mu=args.mu, boundary=args.boundary)
        except ValueError as e:
            print("%s: %s" % (name, e))
            continue
        r = report[name]
        print("%s: %d vertices (%d on the border), %d faces, moved %.4g on average and %.4g at most, volume %.6g -> %.6g" % (
            name, r["vertices"], r["border_vertices"], r["faces"], r["mean_displacement"], r["max_displacement"], r["volume_in"],
            r["volume_out"]))
    with open(os.path.join(args.out_dir, "smooth_mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
