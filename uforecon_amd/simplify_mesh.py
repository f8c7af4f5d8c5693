"""Mesh simplification on the GPU: vertex clustering with quadric placement -- the thinning stage of the mesh route, as
``pcd_filter --voxel_size`` is the point route's; the reference leaves it to Open3D and trimesh.  Every kernel is in
csrc/mesh_simplify.hip (through ``ops.mesh_simplify``); include/ufr.h states every rule, tests/simplify_ref.py restates them in
numpy.

    python -m uforecon_amd.simplify_mesh --mesh_dir OUT/mesh/final --out_dir OUT/mesh/simple
        (--cell C | --target_vertices N | --ratio R) [--placement quadric|mean] [--scans ...] [--ply FILE ...]

reads ``<mesh_dir>/scan<N>.ply`` (with its vertex colours when it has them), writes ``<out_dir>/scan<N>.ply`` and
``<out_dir>/simplify_mesh.json`` with the counts of every scan.  ``--ply`` simplifies the named mesh files instead, each to
``<out_dir>/<file stem>.ply``.  ``--ratio R`` means ``--target_vertices ceil(R * V)``.  The output goes as it stands through
``dtu_eval --mesh_dir``, ``color_mesh --mesh_dir`` and ``render_trajectory --mesh_dir ... --color vertex``.

1. the vertices are binned into cells of edge ``cell`` (Morton keys, one stable sort); one output vertex per occupied cell;
2. every face adds its plane's quadric, weighted by its squared area, to the cells of its corners (one sort, ordered sums);
3. a cell's vertex is the minimiser of its quadric, regularised towards the cell's mean vertex with the weight 2^-10 of the
   quadric's trace, when that lies in the cell and is no worse than the mean; else the mean (``--placement mean``: always);
4. faces whose corners share a cell are dropped, the others are renumbered, and of faces that became equal one is kept.

This is vertex clustering, not edge-collapse decimation: there is no topology guarantee (a thin part can be pinched into
non-manifold edges), normals are not carried (they are recomputed downstream), Open3D's ``simplify_vertex_clustering`` was not
compared against, and no real scan has been simplified.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from .dtu_eval import DTU_SCANS, read_ply


def simplify_mesh(verts, faces, colors=None, cell=None, target_vertices=None, placement="quadric", device="cuda"):
    """A mesh simplified in memory.  ``verts`` (V,3) any float dtype (widened to float64 once), ``faces`` (F,3) integers,
    ``colors`` (V,3) uint8 or None; exactly one of ``cell`` and ``target_vertices``.  Returns the dict of ``ops.mesh_simplify``
    with numpy arrays: ``verts``, ``faces``, ``colors``, ``vertex_map``, ``face_map``, ``placed``, ``count``, and the numbers
    ``cell``, ``clusters``, ``collapsed_faces``, ``duplicate_faces``."""
    import torch

    from . import ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if len(faces) and (faces.min() < -2 ** 31 or faces.max() >= 2 ** 31):
        raise UfrError(f"simplify_mesh: face indices span {faces.min()}..{faces.max()}")
    dev = torch.device(device)
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)
    tc = None
    if colors is not None:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8:
            raise UfrError(f"simplify_mesh: colors {colors.dtype}: expected uint8")
        tc = torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
    out = ops.mesh_simplify(tv, tf, tc, cell=cell, target_vertices=target_vertices, placement=placement)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh_dir", type=str, default="./outputs/mesh/final", help="directory of scan<N>.ply")
    parser.add_argument("--out_dir", type=str, default="./outputs/mesh/simple", help="scan<N>.ply and simplify_mesh.json go here")
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    parser.add_argument("--ply", type=str, nargs="+", default=None,
                        help="simplify these mesh files instead of scan<N>.ply, each to <out_dir>/<file stem>.ply")
    size = parser.add_mutually_exclusive_group(required=True)
    size.add_argument("--cell", type=float, default=None, help="edge of the clustering cells, in the mesh's units")
    size.add_argument("--target_vertices", type=int, default=None, help="the output has at most this many vertices")
    size.add_argument("--ratio", type=float, default=None, help="the output has at most ceil(ratio * V) vertices")
    parser.add_argument("--placement", choices=["quadric", "mean"], default="quadric",
                        help="a cell's vertex: the regularised quadric's minimiser, or always the mean of its vertices")
    return parser


def simplify_file(mesh_path, out_path, cell=None, target_vertices=None, ratio=None, placement="quadric", device="cuda"):
    """One mesh file: reads ``mesh_path``, writes ``out_path`` (with colours when the input has them).  Returns the report
    dict of ``simplify_mesh.json``.  Raises ValueError with one line for a mesh without faces."""
    from .clean_mesh import write_ply
    from .color_mesh import write_ply as write_ply_colors

    verts, faces, colors = read_ply(mesh_path, with_colors=True)
    if faces is None or len(faces) == 0:
        raise ValueError(f"{mesh_path} has no faces")
    if ratio is not None:
        target_vertices = max(1, int(math.ceil(float(ratio) * len(verts))))
    r = simplify_mesh(verts, faces, colors, cell=cell, target_vertices=target_vertices, placement=placement, device=device)
    if r["colors"] is not None:
        write_ply_colors(out_path, r["verts"], r["faces"], r["colors"])
    else:
        write_ply(out_path, r["verts"], r["faces"])
    n_out = int(len(r["verts"]))
    return dict(mesh=mesh_path, placement=placement, vertices_in=int(len(verts)), faces_in=int(len(faces)), vertices_out=n_out,
                faces_out=int(len(r["faces"])), cell=float(r["cell"]), clusters=int(r["clusters"]),
                quadric_share=float(r["placed"].mean()) if n_out else 0.0, collapsed_faces=int(r["collapsed_faces"]),
                duplicate_faces=int(r["duplicate_faces"]), colors=r["colors"] is not None)


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.cell is not None and not (args.cell > 0.0 and args.cell < float("inf")):
        parser.error(f"--cell {args.cell}: must be positive and finite")
    if args.target_vertices is not None and args.target_vertices < 1:
        parser.error(f"--target_vertices {args.target_vertices}: must be >= 1")
    if args.ratio is not None and not 0.0 < args.ratio <= 1.0:
        parser.error(f"--ratio {args.ratio}: must be in (0, 1]")
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
            report[name] = simplify_file(path, os.path.join(args.out_dir, name + ".ply"), cell=args.cell,
                                         target_vertices=args.target_vertices, ratio=args.ratio, placement=args.placement)
        except ValueError as e:
            print("%s: %s" % (name, e))
            continue
        r = report[name]
        print("%s: %d -> %d vertices, %d -> %d faces, cell %g, %.1f %% quadric" % (
            name, r["vertices_in"], r["vertices_out"], r["faces_in"], r["faces_out"], r["cell"], 100.0 * r["quadric_share"]))
    with open(os.path.join(args.out_dir, "simplify_mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
