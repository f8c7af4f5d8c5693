"""DTU mesh cleaning on the GPU: the reference's evaluation/clean_mesh.py (script/clean_mesh.sh), which turns
``<out_dir>/scanN.ply`` into the ``<out_dir>/final/scanN.ply`` that ``uforecon_amd.dtu_eval`` scores, without OpenCV, trimesh,
pyembree or open3d.  Its four stages are HIP kernels (csrc/mesh_clean.hip through ``ops.dilate_mask``,
``ops.mesh_vertex_votes``, ``ops.mesh_first_hit``, ``ops.mesh_face_components``); include/ufr.h states every rule.

    python -m uforecon_amd.clean_mesh --root_dir DTU_TEST --out_dir OUT/mesh [--n_view 3 --set 0 --scale_factor S
                                      --test_ref_view ... --scans ... --min_faces 500]

1. every view's mask is dilated with the 11 x 11 elliptic element and thresholded at > 128 (a colour PNG gives its blue
   channel: the reference reads BGR and takes channel 0);
2. a vertex is kept iff it projects into the dilated mask (or onto the reference's ones border) in more than ``minimal_vis``
   views, a face iff its three vertices are (``clean_mesh_faces_by_mask``);
3. a face is kept iff the ray of some masked pixel of some view hits it first (``clean_mesh_faces_outside_frustum``);
4. components of fewer than ``min_faces`` faces are dropped, and the vertices nothing refers to.

Differences from the reference, all deliberate:
  * the image size comes from the masks, not the hard-coded 1200 x 1600; all masks of a call share one size;
  * the reference's ``mask_faces[values[1:]] = 0`` drops the lowest hit face whenever no ray misses (``values[0]`` is then a
    face, not -1).  That slip is not reproduced: every first-hit face is kept;
  * trimesh merges vertices within a tolerance on load; here only vertices with exactly equal coordinates are one vertex;
  * K and the pose come from the camera file (``K / K[2,2]``, ``inv(E)`` in float64 narrowed to float32), not from
    ``cv.decomposeProjectionMatrix`` of their product: equal up to rounding;
  * ``--scale_factor`` (positive) multiplies all of E, its last row included, by 1 / S.  Stage 2 divides by q.z and stage 3
    normalises ``inv(E)`` by its [3,3] element (as the reference divides the camera centre by its fourth coordinate), so the
    factor cancels in every stage up to rounding.  The flag is accepted and applied as the reference applies it.

Vertices are widened to float64 once on entry, as trimesh holds them.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import cameras
from .dtu_eval import DTU_SCANS, read_ply

TEST_REF_VIEW = [23, 24, 33, 22, 15, 34, 14, 32, 16, 35, 25]
SET1_VIEWS = [43, 42, 44, 33, 34, 32, 45, 23, 41, 24, 31]


def ellipse_half_widths(k: int):
    """Rows of ``cv.getStructuringElement(MORPH_ELLIPSE, (k, k))`` as half-widths (include/ufr.h, ufr_mask_half_widths)."""
    from . import ops

    return ops.mask_half_widths(k)


def read_cam_file(filename, scale_factor=None):
    """(K 3x3, E 4x4) float32 of a ``*_cam.txt`` (the reference's ``read_cam_file``, before it forms P = K4 @ E); E is
    multiplied by 1 / scale_factor when one is given."""
    K, E, _ = cameras.read_cam_file(filename)
    if scale_factor is not None:
        if not scale_factor > 0:
            raise ValueError(f"scale_factor {scale_factor}: must be positive")
        E = E * np.float32(1.0 / scale_factor)
    return K, E


def read_mask(filename):
    """(H,W) uint8: the image itself when it is grey, the blue channel of a colour image"""
    from PIL import Image

    img = Image.open(filename)
    if img.mode not in ("L", "RGB"):
        img = img.convert("RGB" if img.mode in ("RGBA", "P", "CMYK") else "L")
    a = np.array(img, dtype=np.uint8)
    return np.ascontiguousarray(a if a.ndim == 2 else a[:, :, 2])


def projection(K, E):
    """P = K4 @ E in float32, as ``read_cam_file`` of the reference returns it"""
    K4 = np.float32(np.diag([1, 1, 1, 1]))
    K4[:3, :3] = np.asarray(K, np.float32)
    return K4 @ np.asarray(E, np.float32)


def ray_camera(K, E):
    """(k_inv 3x3, c2w 4x4) float32: what the reference hands ``gen_rays_from_single_image``"""
    import torch

    K64 = np.asarray(K, np.float32).astype(np.float64)
    k_inv = torch.inverse(torch.from_numpy(K64 / K64[2, 2]).float()).numpy()
    c2w = np.linalg.inv(np.asarray(E, np.float32).astype(np.float64))
    return k_inv, (c2w / c2w[3, 3]).astype(np.float32)      # c2w[3,3] is 1 unless E was scaled as a whole


def write_ply(filename, verts, faces):
    """binary little-endian PLY: float x / y / z, ``list uchar int`` faces"""
    verts = np.asarray(verts).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    vrec = np.ascontiguousarray(verts.astype("<f4"))
    frec = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = faces
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(vrec), len(frec)))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def _compact(keep):
    """new index of every kept item, in the original order"""
    import torch

    return torch.cumsum(keep.to(torch.int64), 0) - 1


def clean_mesh(verts, faces, cams, masks, minimal_vis=1, mask_dilated_size=11, min_faces=500, return_stages=False,
               largest_only=False, device="cuda"):
    """The cleaned ``(verts (V',3) float64, faces (F',3) int32)`` as numpy arrays.  ``verts`` (V,3) any float dtype, ``faces``
    (F,3) integers; ``cams``: one ``(K 3x3, E 4x4)`` pair per view as in a ``*_cam.txt``; ``masks``: one (H,W) uint8 image per
    view, all of one size.  An empty mesh, masks without a ray, or nothing surviving give empty arrays.  ``largest_only``
    keeps only the largest surviving component (the reference's unused ``clean_outliers``), ties to the lowest label.

    ``return_stages``: also a dict with ``votes`` (V,), the stage-2 mesh ``verts2`` / ``faces2``, ``face_ids`` (one (H,W) int32
    image per view, indices into ``faces2``), ``faces3`` (the first-hit faces), ``labels`` (per face of ``faces3``: the lowest
    face index of its component, -1 without adjacency) and ``rounds`` (union-find rounds)."""
    import torch

    from . import ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    cams, masks = list(cams), [np.asarray(m) for m in masks]
    if len(cams) != len(masks) or not cams:
        raise UfrError(f"clean_mesh: {len(cams)} cameras, {len(masks)} masks (need one mask per camera, at least one)")
    for m in masks:
        if m.ndim != 2 or m.dtype != np.uint8 or m.shape != masks[0].shape:
            raise UfrError(f"clean_mesh: masks must be (H, W) uint8 images of one size, got {[(x.shape, str(x.dtype)) for x in masks]}")
    V, F = len(verts), len(faces)
    if F and (V == 0 or faces.min() < 0 or faces.max() >= V):
        raise UfrError(f"clean_mesh: face indices span {faces.min()}..{faces.max()}, the mesh has {V} vertices")
    dev = torch.device(device)
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)

    # 1. dilated masks
    dil = torch.stack([ops.dilate_mask(torch.from_numpy(np.ascontiguousarray(m)).to(dev), mask_dilated_size) for m in masks])
    # 2. votes, and the compaction of the kept vertices and faces
    P = torch.from_numpy(np.stack([projection(K, E)[:3] for K, E in cams])).to(dev)
    votes = ops.mesh_vertex_votes(tv, P, dil)
    vkeep = votes > minimal_vis
    tfl = tf.long()
    fkeep = vkeep[tfl[:, 0]] & vkeep[tfl[:, 1]] & vkeep[tfl[:, 2]] if F else torch.zeros(0, dtype=torch.bool, device=dev)
    v2 = tv[vkeep].contiguous()
    f2 = _compact(vkeep)[tfl[fkeep]].to(torch.int32).contiguous().reshape(-1, 3)
    # 3. first-hit faces over the views
    hit = torch.zeros(len(f2), dtype=torch.uint8, device=dev)
    face_ids = []
    for (K, E), m in zip(cams, dil):
        k_inv, c2w = ray_camera(K, E)
        if len(v2):
            fid, hit = ops.mesh_first_hit(v2, f2, k_inv, c2w, m, hit)
        else:
            fid = torch.full(tuple(m.shape), -1, dtype=torch.int32, device=dev)
        face_ids.append(fid)
    f3 = f2[hit != 0].contiguous()
    # 4. components
    if len(f3):
        labels, rounds = ops.mesh_face_components(v2, f3, return_rounds=True)
    else:
        labels, rounds = torch.zeros(0, dtype=torch.int32, device=dev), 0
    size = torch.bincount(labels[labels >= 0].long(), minlength=max(len(f3), 1))
    keep = (labels >= 0) & (size[labels.clamp(min=0).long()] >= min_faces)
    if largest_only and bool(keep.any()):
        cand = torch.where(size >= max(min_faces, 1), size, torch.zeros_like(size)).cpu().numpy()
        keep &= labels == int(cand.argmax())                       # numpy's argmax: the first maximum, the lowest label
    f4 = f3[keep]
    used = torch.zeros(len(v2), dtype=torch.bool, device=dev)
    used[f4.long().reshape(-1)] = True
    out_v = v2[used].cpu().numpy()
    out_f = _compact(used)[f4.long()].to(torch.int32).reshape(-1, 3).cpu().numpy()
    if not return_stages:
        return out_v, out_f
    stages = dict(votes=votes.cpu().numpy(), verts2=v2.cpu().numpy(), faces2=f2.cpu().numpy(),
                  face_ids=[f.cpu().numpy() for f in face_ids], faces3=f3.cpu().numpy(), labels=labels.cpu().numpy(), rounds=rounds)
    return out_v, out_f, stages


def make_parser():
    """The reference's flags and defaults (clean_mesh.py:284-293), plus --scans and --min_faces."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--root_dir", dest="root_dir", type=str, default="./dtu_test", help="dataset")
    parser.add_argument("--out_dir", dest="out_dir", type=str, default="./outputs/mesh", help="directory of to save test result")
    parser.add_argument("--n_view", dest="n_view", type=int, default=3)
    parser.add_argument("--set", dest="set", type=int, default=0)
    parser.add_argument("--scale_factor", type=float)
    parser.add_argument("--test_ref_view", type=int, nargs="+", default=TEST_REF_VIEW)
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    parser.add_argument("--min_faces", type=int, default=500, help="smallest component kept (the reference: 500)")
    return parser


def clean_scan(root_dir, out_dir, scan, imgs_idx, scale_factor=None, min_faces=500, mask_kernel_size=11):
    """One scan of the reference's main loop: reads ``<out_dir>/scan{N}.ply``, the cameras and masks of ``imgs_idx``; writes
    ``final/clean_{N:03d}.ply`` (stage 2), ``final/scan{N}_raw.ply`` (stage 3) and ``final/scan{N}.ply``."""
    verts, faces = read_ply(os.path.join(out_dir, "scan%d.ply" % scan))
    if faces is None:
        faces = np.zeros((0, 3), np.int32)
    cams = [read_cam_file(os.path.join(root_dir, "cameras/{:0>8}_cam.txt".format(v)), scale_factor) for v in imgs_idx]
    masks = [read_mask(os.path.join(root_dir, "scan{}/mask/{:0>3}.png".format(scan, v))) for v in imgs_idx]
    v4, f4, st = clean_mesh(verts, faces, cams, masks, minimal_vis=1, mask_dilated_size=mask_kernel_size, min_faces=min_faces,
                            return_stages=True)
    final = os.path.join(out_dir, "final")
    write_ply(os.path.join(final, "clean_%03d.ply" % scan), st["verts2"], st["faces2"])
    print(f"Surfaces/Kept: {len(st['faces2'])}/{len(st['faces3'])}")
    write_ply(os.path.join(final, "scan%d_raw.ply" % scan), st["verts2"], st["faces3"])
    write_ply(os.path.join(final, "scan%d.ply" % scan), v4, f4)
    return v4, f4


def main(argv=None):
    args = make_parser().parse_args(argv)
    view_list = args.test_ref_view if args.set == 0 else SET1_VIEWS
    imgs_idx = view_list[:args.n_view]
    os.makedirs(os.path.join(args.out_dir, "final"), exist_ok=True)
    for scan in args.scans:
        print("processing scan%d" % scan)
        if not os.path.exists(os.path.join(args.out_dir, "scan%d.ply" % scan)):
            print("scan%d is empty" % scan)
            continue
        clean_scan(args.root_dir, args.out_dir, scan, imgs_idx, args.scale_factor, args.min_faces)
        print("finish processing scan%d" % scan)


if __name__ == "__main__":
    sys.exit(main())
