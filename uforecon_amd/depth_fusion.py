"""Depth-map fusion to a point cloud by geometric consistency: the reference's code1/encoder_utils/depth_fusion.py
(run by script/depth_fusion.sh) on the GPU.  The per-pixel work is csrc/depth_fusion.hip (``ops.depth_consistency``,
``ops.depth_points``); this module forms the small matrices, reads and writes the reference's files, and is the command
line:

    python -m uforecon_amd.depth_fusion --root_dir OUT [--dataset_dir DTU_TEST --full_fusion] [--n_view 3] ...

It reads what ``model.save_depth_outputs`` writes (``depth/<scan>/<%08d>.npy`` dicts, ``rgb/<scan>/<%08d>.jpg``) and writes
``<root_dir>/<scan>/mask/<%08d>.png`` and ``<root_dir>/pcd/<scan>.ply``, which ``python -m uforecon_amd.dtu_eval --mode pcd``
scores.

The PLY layout is the one ``plyfile`` writes by default for the reference's structured array: ``binary_little_endian 1.0``,
one ``vertex`` element with ``float x y z`` and ``uchar red green blue``, 15 bytes per vertex.  plyfile was not at hand when
this was written: the layout follows its documentation and is NOT byte-compared with a plyfile-written file.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import cameras


def read_pair_file(filename):
    """[(ref_view, [src_view ...])] of an MVSNet ``pair.txt``; views without sources are dropped (depth_fusion.py:14-24)."""
    return [(ref, srcs) for ref, srcs in cameras.read_pair_file(filename) if srcs]


def pair_matrices(K_ref, E_ref, K_src, E_src) -> np.ndarray:
    """The 68 doubles of one (reference, source) pair for ``ops.depth_consistency``: the reference's own numpy expressions in
    the dtypes the inputs arrive in (float32 inputs give float32 LAPACK inverses and products, as there), widened after."""
    parts = (np.linalg.inv(K_ref), np.matmul(E_src, np.linalg.inv(E_ref)), K_src, np.linalg.inv(K_src),
             np.matmul(E_ref, np.linalg.inv(E_src)), K_ref)
    shapes = ((3, 3), (4, 4), (3, 3), (3, 3), (4, 4), (3, 3))
    for m, sh in zip(parts, shapes):
        if np.shape(m) != sh:
            raise ValueError(f"pair_matrices: intrinsics must be 3x3 and extrinsics 4x4 (got a {np.shape(m)} where {sh} belongs)")
    return np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in parts])


def fuse_views(depths, intrinsics, extrinsics, colors, pairs, geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2,
               return_details=False):
    """Fuse depth maps in memory.  ``depths[v]`` (H,W) float32, ``intrinsics[v]`` 3x3, ``extrinsics[v]`` 4x4 (world to camera),
    ``colors[v]`` (H,W,3) uint8, indexed by view (sequences or dicts; views may differ in size); ``pairs`` a list of
    ``(ref, [src ...])``.  Returns ``xyz`` float32 (N,3) and ``rgb`` uint8 (N,3), the reference views' points concatenated in
    the order of ``pairs`` and in row-major pixel order inside a view, and ``masks``, one (H,W) bool array per entry of
    ``pairs``.  Every depth map is uploaded once, however many pairs use it.  ``return_details``: also a list of dicts with
    each reference view's ``geo_mask_sum`` (int32), ``depth_est_averaged`` (float64) and ``pair_masks`` ((S,H,W) bool)."""
    import torch

    from . import ops

    dev = torch.device("cuda")
    d_depth, d_color = {}, {}

    def depth_of(v):
        if v not in d_depth:
            a = np.asarray(depths[v])
            if a.dtype != np.float32 or a.ndim != 2:
                raise ValueError(f"fuse_views: depth of view {v} is {a.dtype} {a.shape}, expected float32 (H, W)")
            d_depth[v] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return d_depth[v]

    def color_of(v):
        if v not in d_color:
            a = np.asarray(colors[v])
            if a.dtype != np.uint8 or a.shape != (*np.shape(depths[v]), 3):
                raise ValueError(f"fuse_views: colour of view {v} is {a.dtype} {a.shape}, expected uint8 (H, W, 3) of its depth map")
            d_color[v] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return d_color[v]

    out_xyz, out_rgb, masks, details = [], [], [], []
    for ref, srcs in pairs:
        srcs = list(srcs)
        if not 1 <= len(srcs) <= ops.DEPTH_MAX_SOURCES:
            raise ValueError(f"fuse_views: view {ref} has {len(srcs)} source views (must be 1 .. {ops.DEPTH_MAX_SOURCES})")
        K, E = intrinsics[ref], extrinsics[ref]
        mats = np.stack([pair_matrices(K, E, intrinsics[s], extrinsics[s]) for s in srcs])
        res = ops.depth_consistency(depth_of(ref), [depth_of(s) for s in srcs], torch.from_numpy(mats).to(dev), geo_pixel_thres,
                                    geo_depth_thres, geo_mask_thres, return_pair_masks=return_details)
        mask_sum, mask, avg = res[:3]
        xyz, rgb = ops.depth_points(mask, avg, color_of(ref), np.linalg.inv(K), np.linalg.inv(E))
        out_xyz.append(xyz)
        out_rgb.append(rgb)
        masks.append(mask.cpu().numpy().astype(bool))
        if return_details:
            details.append(dict(geo_mask_sum=mask_sum.cpu().numpy(), depth_est_averaged=avg.cpu().numpy(),
                                pair_masks=res[3].cpu().numpy().astype(bool)))
    xyz = torch.cat(out_xyz).cpu().numpy() if out_xyz else np.zeros((0, 3), np.float32)
    rgb = torch.cat(out_rgb).cpu().numpy() if out_rgb else np.zeros((0, 3), np.uint8)
    return (xyz, rgb, masks, details) if return_details else (xyz, rgb, masks)


def write_ply(filename, xyz, rgb):
    """The cloud as plyfile writes the reference's vertex array (see the module docstring)."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    rec = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = xyz[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = rgb[:, k]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(rec))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def save_mask(filename, mask):
    from PIL import Image

    assert mask.dtype == np.bool_
    Image.fromarray(mask.astype(np.uint8) * 255).save(filename)


def filter_depth(root_dir, scan, dataset_dir=None, n_view=3, geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2,
                 full_fusion=False):
    """The reference's ``filter_depth`` (depth_fusion.py:93-231) on the reference's files.  Without ``full_fusion`` the views
    are 0 .. n_view-1 and each one's sources are the others (``views[:]`` with ``pop(ref_view)``); with it, the views and
    sources of ``<dataset_dir>/pair.txt`` (``dataset_dir`` is needed only then).  Writes the masks and the cloud; returns
    ``(xyz, rgb, masks)``."""
    from PIL import Image

    if full_fusion:
        if dataset_dir is None:
            raise ValueError("filter_depth: full_fusion needs dataset_dir (the directory of pair.txt)")
        pairs = read_pair_file(os.path.join(dataset_dir, "pair.txt"))
    else:
        views = list(range(n_view))
        pairs = []
        for ref in views:
            srcs = views[:]
            srcs.pop(ref)
            pairs.append((ref, srcs))
    depths, K, E, colors = {}, {}, {}, {}
    for ref, srcs in pairs:
        for v in [ref] + list(srcs):
            if v not in depths:
                d = np.load(os.path.join(root_dir, "depth", scan, "{:0>8}.npy".format(v)), allow_pickle=True).item()
                depths[v], K[v], E[v] = d["depth"], d["intrinsic"], d["extrinsic"]
        if ref not in colors:
            colors[ref] = np.array(Image.open(os.path.join(root_dir, "rgb", scan, "{:0>8}.jpg".format(ref))), dtype=np.uint8)
    xyz, rgb, masks = fuse_views(depths, K, E, colors, pairs, geo_pixel_thres, geo_depth_thres, geo_mask_thres)
    os.makedirs(os.path.join(root_dir, scan, "mask"), exist_ok=True)
    for (ref, _), mask in zip(pairs, masks):
        save_mask(os.path.join(root_dir, scan, "mask/{:0>8}.png".format(ref)), mask)
        print("processing {}, ref-view{:0>2}, geo_mask:{:3f}".format(scan, ref, mask.mean()))
    os.makedirs(os.path.join(root_dir, "pcd"), exist_ok=True)
    plyfilename = os.path.join(root_dir, "pcd", "{}.ply".format(scan))
    write_ply(plyfilename, xyz, rgb)
    print("saving the final model to", plyfilename)
    return xyz, rgb, masks


def make_parser():
    """The reference's flags and defaults (depth_fusion.py:236-250)."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--dataset", dest="dataset", type=str, default="DTU", help="dataset name")
    parser.add_argument("--dataset_dir", dest="dataset_dir", type=str, help="directory of dataset")
    parser.add_argument("--root_dir", dest="root_dir", type=str, help="directory of srdf volumes")
    parser.add_argument("--n_view", dest="n_view", type=int, default=3)
    parser.add_argument("--geo_pixel_thres", type=float, default=1, help="pixel threshold for geometric consistency filtering")
    parser.add_argument("--geo_depth_thres", type=float, default=0.01, help="depth threshold for geometric consistency filtering")
    parser.add_argument("--geo_mask_thres", type=int, default=2, help="number of consistent views for geometric consistency filtering")
    parser.add_argument("--set", dest="set", type=int, default=0)
    parser.add_argument("--full_fusion", dest="full_fusion", action="store_true", help="fuse all the depth maps")
    return parser


def main(argv=None):
    args = make_parser().parse_args(argv)
    scans = [i for i in os.listdir(args.root_dir) if i[:4] == "scan"]
    print("found scans:", scans)
    os.makedirs(os.path.join(args.root_dir, "pcd"), exist_ok=True)
    for scan in scans:
        filter_depth(args.root_dir, scan, args.dataset_dir, args.n_view, args.geo_pixel_thres, args.geo_depth_thres,
                     args.geo_mask_thres, args.full_fusion)


if __name__ == "__main__":
    main()
