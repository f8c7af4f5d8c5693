"""Feature-preserving mesh denoising on the GPU: a bilateral filter of the face normals, then vertices moved to the filtered
normals -- the sibling of ``smooth_mesh`` that keeps a crease where Taubin steps round it; the reference leaves it to Open3D and
trimesh.  Every kernel is in csrc/mesh_denoise.hip (through ``ops.mesh_denoise``); include/ufr.h states every rule,
tests/denoise_ref.py restates them in numpy.

    python -m uforecon_amd.denoise_mesh --mesh_dir OUT/mesh/final --out_dir OUT/mesh/denoise [--normal_iterations 5]
        [--vertex_iterations 10] [--sigma_s S] [--sigma_r 0.35] [--boundary fixed|free] [--scans ...] [--ply FILE ...]

reads ``<mesh_dir>/scan<N>.ply`` (with its vertex colours when it has them), writes ``<out_dir>/scan<N>.ply`` and
``<out_dir>/denoise_mesh.json`` with the counts, the sigmas used, the displacement, the mean turn of the normals and the
enclosed volume of every scan.  ``--ply`` denoises the named mesh files instead, each to ``<out_dir>/<file stem>.ply``.  Only
the vertex positions change: faces, vertex order and colours pass through, so the output goes as it stands through
``simplify_mesh``, ``color_mesh``, ``dtu_eval`` and ``render_trajectory``.

1. every face gets a unit normal, an area and a centroid from the input positions; a face that names a vertex twice, or has
   no area, is dead: nobody's neighbour, never filtered;
2. a face's neighbours are the faces that share a vertex with it, each once, itself first (Zheng et al. 2011, local scheme);
3. one normal step replaces a normal by the normalised sum of its neighbours' normals, each weighed by its area, by
   ``k(|dc|^2 / 2 sigma_s^2)`` of the distance between centroids and by ``k(|dn|^2 / 2 sigma_r^2)`` of the difference of normals;
   ``k(u) = (1 - u/256)^256`` stands in for ``exp(-u)`` so that numpy and the device agree in every bit;
4. one vertex step moves a vertex by the mean, over its faces, of the face normal times the distance from the vertex to the
   face's centroid plane (Sun et al. 2007); a border vertex stays where it is unless ``--boundary free``.

``sigma_s`` defaults to the mean edge length of the mesh; ``sigma_r`` = 0.35 is the chord of about 20 degrees, the turn at which
a neighbour weighs e^-1/2: a stated choice, not tuned on a scan.  It has to grow with the noise: noise of a third of an edge
defeats 0.35.  Open3D and MeshLab were not compared against, and no real scan has been denoised.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from .dtu_eval import DTU_SCANS, read_ply
from .smooth_mesh import signed_volume

SIGMA_R = 0.35


def _face_normals(verts, faces):
    """(normals (F,3), live (F,)) on the host: float64 cross products; a dead face's row is not to be used"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(all="ignore"):
        m = np.cross(p1 - p0, p2 - p0)
        nf = np.linalg.norm(m, axis=1)
        live = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]) & (nf > 0) & np.isfinite(nf)
        return m / np.where(live, nf, 1.0)[:, None], live


def mean_edge_length(verts, faces):
    """the default ``sigma_s``: the mean of the three edge lengths of every live face (float64 on the host); tests/denoise_ref.py
    holds the same expression"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(all="ignore"):
        nf = np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
    live = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]) & (nf > 0) & np.isfinite(nf)
    edges = np.stack([p1 - p0, p2 - p1, p0 - p2])[:, live]
    return float(np.mean(np.linalg.norm(edges, axis=-1)))


def denoise_mesh(verts, faces, normal_iterations=5, vertex_iterations=10, sigma_s=None, sigma_r=SIGMA_R, boundary="fixed", pinned=None,
                 device="cuda"):
    """A mesh denoised in memory.  ``verts`` (V,3) any float dtype (widened to float64 once), ``faces`` (F,3) integers,
    ``pinned`` (V,) uint8 or None; ``sigma_s`` None: the mean edge length over the live faces; the other arguments are those of
    ``ops.mesh_denoise``.  Returns its dict with numpy arrays -- ``verts`` (V,3) float64, ``normals`` (F,3) float64, ``border``
    (V,) uint8 -- and ``sigma_s``, the value used."""
    import torch

    from . import ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if len(faces) and (faces.min() < -2 ** 31 or faces.max() >= 2 ** 31):
        raise UfrError(f"denoise_mesh: face indices span {faces.min()}..{faces.max()}")
    if len(faces) and (len(verts) == 0 or faces.min() < 0 or faces.max() >= len(verts)):
        raise UfrError(f"denoise_mesh: face indices span {faces.min()}..{faces.max()}, the mesh has {len(verts)} vertices")
    if sigma_s is None:
        sigma_s = mean_edge_length(verts, faces) if len(faces) else 1.0
        if not sigma_s > 0.0:                              # no live face (np.mean of nothing is NaN): nothing will be filtered
            sigma_s = 1.0
    dev = torch.device(device)
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)
    tp = None
    if pinned is not None:
        pinned = np.asarray(pinned)
        if pinned.dtype != np.uint8:
            raise UfrError(f"denoise_mesh: pinned {pinned.dtype}: expected uint8")
        tp = torch.from_numpy(np.ascontiguousarray(pinned)).to(dev)
    out = ops.mesh_denoise(tv, tf, normal_iterations=normal_iterations, vertex_iterations=vertex_iterations, sigma_s=sigma_s,
                           sigma_r=sigma_r, boundary=boundary, pinned=tp)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["sigma_s"] = float(sigma_s)
    return out


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh_dir", type=str, default="./outputs/mesh/final", help="directory of scan<N>.ply")
    parser.add_argument("--out_dir", type=str, default="./outputs/mesh/denoise", help="scan<N>.ply and denoise_mesh.json go here")
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    parser.add_argument("--ply", type=str, nargs="+", default=None,
                        help="denoise these mesh files instead of scan<N>.ply, each to <out_dir>/<file stem>.ply")
    parser.add_argument("--normal_iterations", type=int, default=5, help="steps of the bilateral normal filter")
    parser.add_argument("--vertex_iterations", type=int, default=10, help="steps that move the vertices to the filtered normals")
    parser.add_argument("--sigma_s", type=float, default=None, help="the spatial scale, above 0 (default: the mesh's mean edge length)")
    parser.add_argument("--sigma_r", type=float, default=SIGMA_R,
                        help="the scale of the difference of unit normals, above 0 (0.35: the chord of about 20 degrees)")
    parser.add_argument("--boundary", choices=["fixed", "free"], default="fixed", help="fixed: border vertices stay where they are")
    return parser


def denoise_file(mesh_path, out_path, normal_iterations=5, vertex_iterations=10, sigma_s=None, sigma_r=SIGMA_R, boundary="fixed",
                 device="cuda"):
    """One mesh file: reads ``mesh_path``, writes ``out_path`` (with colours when the input has them).  Returns the report
    dict of ``denoise_mesh.json``.  Raises ValueError with one line for a mesh without faces."""
    from .clean_mesh import write_ply
    from .color_mesh import write_ply as write_ply_colors

    verts, faces, colors = read_ply(mesh_path, with_colors=True)
    if faces is None or len(faces) == 0:
        raise ValueError(f"{mesh_path} has no faces")
    r = denoise_mesh(verts, faces, normal_iterations=normal_iterations, vertex_iterations=vertex_iterations, sigma_s=sigma_s,
                     sigma_r=sigma_r, boundary=boundary, device=device)
    if colors is not None:
        write_ply_colors(out_path, r["verts"], faces, colors)
    else:
        write_ply(out_path, r["verts"], faces)
    moved = np.linalg.norm(r["verts"] - np.asarray(verts, np.float64), axis=1)
    n_in, live = _face_normals(verts, faces)
    turn = np.degrees(np.arccos(np.clip(np.einsum("ij,ij->i", n_in[live], r["normals"][live]), -1.0, 1.0)))
    return dict(mesh=mesh_path, normal_iterations=int(normal_iterations), vertex_iterations=int(vertex_iterations),
                sigma_s=float(r["sigma_s"]), sigma_r=float(sigma_r), boundary=boundary, vertices=int(len(verts)), faces=int(len(faces)),
                border_vertices=int(r["border"].sum()), mean_displacement=float(moved.mean()), max_displacement=float(moved.max()),
                mean_normal_turn_deg=float(turn.mean()) if len(turn) else 0.0, volume_in=signed_volume(verts, faces),
                volume_out=signed_volume(r["verts"], faces), colors=colors is not None)


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.normal_iterations < 0:
        parser.error(f"--normal_iterations {args.normal_iterations}: must be >= 0")
    if args.vertex_iterations < 0:
        parser.error(f"--vertex_iterations {args.vertex_iterations}: must be >= 0")
    if args.sigma_s is not None and not (0.0 < args.sigma_s < float("inf")):
        parser.error(f"--sigma_s {args.sigma_s}: must be finite and above 0")
    if not (0.0 < args.sigma_r < float("inf")):
        parser.error(f"--sigma_r {args.sigma_r}: must be finite and above 0")
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
            report[name] = denoise_file(path, os.path.join(args.out_dir, name + ".ply"), normal_iterations=args.normal_iterations,
                                        vertex_iterations=args.vertex_iterations, sigma_s=args.sigma_s, sigma_r=args.sigma_r,
                                        boundary=args.boundary)
        except ValueError as e:
            print("%s: %s" % (name, e))
            continue
        r = report[name]
        print("%s: %d vertices (%d on the border), %d faces, sigma_s %.4g, normals turned %.3g degrees on average, moved %.4g on "
              "average and %.4g at most, volume %.6g -> %.6g" % (
                  name, r["vertices"], r["border_vertices"], r["faces"], r["sigma_s"], r["mean_normal_turn_deg"], r["mean_displacement"],
                  r["max_displacement"], r["volume_in"], r["volume_out"]))
    with open(os.path.join(args.out_dir, "denoise_mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
