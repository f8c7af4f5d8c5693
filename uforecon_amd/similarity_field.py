"""The similarity field of a scan: what the cross-view matching features alone say about where the surface is, before any
transformer or compositor -- the reference's `UFORecon.extract_similarity` / `extract_fields` (code1/model.py:844-911).

    python -m uforecon_amd.similarity_field --set 0 --volume_type correlation --depth_pos_encoding --mvs_depth_guide 1 \\
        --explicit_similarity --test_n_view 3 --test_ref_view 23 24 33 --test_dir DTU_TEST --load_ckpt uforecon.ckpt --out_dir OUT \\
        --resolution 512 --threshold 0.99

The flags, loaders and refusals are `python -m uforecon_amd.extract_geometry`'s (`--test_general` included), plus
`--resolution`, `--threshold`, `--bound_min / --bound_max`, `--min_views` and `--save_field`.  The field needs one view group
per scan, so the command runs ONE batch per scan, the first render view, and writes `<out_dir>/sim_<scan>_<resolution>.ply`
(with `--save_field` also `sim_<scan>_<resolution>.npy`, the (X,Y,Z) float32 field).

The field is `ops.similarity_field` (csrc/similarity_field.hip): per voxel the mean over the view pairs and the 8 channel
groups of the pair similarity the gather feeds the ray transformer, sampled with border clamping and without a depth mask.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from . import ops


def similarity_field(frame, bound_min=(-1., -1., -1.), bound_max=(1., 1., 1.), resolution=512, min_views=0, return_visibility=False):
    """`ops.similarity_field` under the reference's defaults: ``u`` (X,Y,Z) fp32 on the device, allocated NaN-filled (an
    unwritten voxel cannot pass for a value); with ``return_visibility`` also ``n_vis`` (X,Y,Z) uint8."""
    return ops.similarity_field(frame, bound_min, bound_max, resolution, min_views=min_views, return_visibility=return_visibility)


def field_mesh(u, bound_min, bound_max, level=0.99):
    """The surface ``u = level`` of a field as (verts (V,3) fp32 in scene coordinates, faces (F,3) int32, normals (V,3) fp32),
    device tensors.  It is ``ops.marching_cubes(-u, -level)``: occupied (u > level) is inside, as the negative side of a TSDF
    is, so the faces wind the way the TSDF meshes do and the normals point out of the occupied region; the negation is exact.
    Vertices map from voxel indices to the scene as ``v / (dim - 1) * (max - min) + min`` (the line the reference leaves
    commented out, model.py:886)."""
    verts, faces, normals = ops.marching_cubes(-u, -float(level))
    lo = torch.as_tensor(bound_min, dtype=torch.float32).reshape(3).to(u.device)
    hi = torch.as_tensor(bound_max, dtype=torch.float32).reshape(3).to(u.device)
    steps = torch.tensor([d - 1 for d in u.shape], dtype=torch.float32, device=u.device)
    return verts / steps * (hi - lo) + lo, faces, normals


def resolution_tag(resolution) -> str:
    """What stands for the resolution in a file name: "512", or "64x32x16" for three different extents."""
    if isinstance(resolution, int):
        return str(resolution)
    r = [int(v) for v in resolution]
    return str(r[0]) if r[0] == r[1] == r[2] else "x".join(str(v) for v in r)


def scan_name(batch) -> str:
    """The scan field of a batch's meta ("dtu-scan24-00000000" -> "scan24"), as the reference reads it (model.py:883)."""
    return batch["meta"][0].split("-")[1]


def write_mesh(filename, verts, faces, normals):
    """`tsdf.meshwrite` (ASCII PLY, the layout of the TSDF meshes) with one grey for every vertex: the field has no colour."""
    from . import tsdf

    v = verts.cpu().numpy()
    tsdf.meshwrite(filename, v, faces.cpu().numpy(), normals.cpu().numpy(), np.full((len(v), 3), 200, np.uint8))


def main(argv=None):
    from . import extract_geometry as EG

    parser = EG.make_parser()
    parser.description = __doc__.split("\n")[0]
    parser.add_argument("--resolution", type=int, default=512, help="voxels per axis of the field")
    parser.add_argument("--threshold", type=float, default=0.99, help="level of the mesh (the reference's fixed 0.99)")
    parser.add_argument("--bound_min", type=float, nargs=3, default=[-1., -1., -1.], help="lower corner of the grid")
    parser.add_argument("--bound_max", type=float, nargs=3, default=[1., 1., 1.], help="upper corner of the grid")
    parser.add_argument("--min_views", type=int, default=0, help="voxels seen by fewer views get -1 (0: the reference, no masking)")
    parser.add_argument("--save_field", action="store_true", help="also write sim_<scan>_<resolution>.npy")
    args = EG.parse_args(argv, parser)
    why = EG.unimplemented(args)
    if why is None and not (args.test_dir and args.out_dir):
        why = "--test_dir and --out_dir are required"
    if why is None and args.resolution < 2:
        why = f"--resolution {args.resolution}: at least 2"
    if why is None and not 0 <= args.min_views <= args.test_n_view:
        why = f"--min_views {args.min_views}: 0 .. --test_n_view {args.test_n_view}"
    if why is not None:
        parser.error(why)
    args.img_wh, args.original_img_wh = EG.resolve_img_wh(args)
    args.extract_geometry = True
    dev = torch.device("cuda:0")
    scans = []          # every scan is opened before the model is built: a missing file costs nothing
    if args.test_general:
        from .general_scan import GeneralScan

        if args.img_wh[0] % EG.IMG_MULTIPLE or args.img_wh[1] % EG.IMG_MULTIPLE:
            parser.error(f"--img_wh {args.img_wh[0]} {args.img_wh[1]}: width and height must be multiples of {EG.IMG_MULTIPLE}")
        for scan in args.test_scan:
            try:
                scans.append((scan, GeneralScan(args.test_dir, scan, n_views=args.test_n_view, test_ref_view=args.test_ref_view,
                                                dataset=args.dataset, use_mask=args.use_mask, img_wh=args.img_wh, device="cuda:0")))
            except FileNotFoundError as e:
                parser.error(f"{scan}: {e.filename} is missing under --test_dir {args.test_dir}")
            except ValueError as e:
                parser.error(f"{scan}: --test_n_view {args.test_n_view}: {e}")
    else:
        from .dtu_scan import DtuScan

        for scan in args.scans:
            try:
                scans.append(("scan%d" % scan, DtuScan(args.test_dir, "scan%d" % scan, n_views=args.test_n_view, img_wh=args.img_wh,
                                                       original_img_wh=args.original_img_wh, set=args.set,
                                                       test_view_pair=args.test_ref_view, device=dev)))
            except FileNotFoundError as e:
                parser.error(f"scan{scan}: {e.filename} is missing under --test_dir {args.test_dir}")
    net = EG.load_net(args, dev)
    for name, frames in scans:
        try:
            batch = frames[0]
        except FileNotFoundError as e:
            parser.error(f"{name}: {e.filename} is missing under --test_dir {args.test_dir}")
        u = net.extract_similarity(batch, bound_min=args.bound_min, bound_max=args.bound_max, resolution=args.resolution,
                                   threshold=args.threshold, min_views=args.min_views, out_dir=args.out_dir)
        stem = os.path.join(args.out_dir, "sim_%s_%s" % (scan_name(batch), resolution_tag(args.resolution)))
        if args.save_field:
            np.save(stem + ".npy", u.cpu().numpy())
        print("%s -> %s.ply" % (name, stem))
    return 0


if __name__ == "__main__":
    sys.exit(main())
