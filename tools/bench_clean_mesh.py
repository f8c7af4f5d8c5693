"""Benchmark of DTU mesh cleaning (uforecon_amd/clean_mesh.py) on a DTU-sized case: the marching-cubes mesh of a synthetic
sphere TSDF at 1.5 mm voxels (about 3 M faces), 3 views of 1200 x 1600 on an arc, disc masks a little larger than the sphere.
  * kernels: HIP events around every launch (ufr_profile_*), summed per stage -- dilation, votes, first hit (the key-image
    reset, both triangle kernels and the resolve, three views), components (edge keys, pair marking, union-find rounds);
  * end to end: ``clean_mesh`` wall time, which adds the uploads, torch's unique / sort / compaction, the per-round
    synchronisations and the copy of the result to the host.
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
from uforecon_amd import clean_mesh as CM, ops  # noqa: E402

VOXEL = 1.5


def sphere_mesh(radius_vox=280, device="cuda"):
    n = 2 * radius_vox + 16
    ax = torch.arange(n, dtype=torch.float32, device=device) - (n - 1) / 2
    vol = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - radius_vox
    verts, faces, _ = ops.marching_cubes(vol.contiguous(), 0.0)
    return ((verts.double() - (n - 1) / 2) * VOXEL).cpu().numpy(), faces.cpu().numpy()


def scene(radius_mm, H=1200, W=1600, focal=2900.0):
    dist = focal * radius_mm / 500.0                          # the sphere's image is about 500 pixels in radius
    K = np.array([[focal, 0, W / 2 + 0.37], [0, focal, H / 2 + 0.21], [0, 0, 1]], np.float32)
    cams, masks = [], []
    ys, xs = np.mgrid[:H, :W]
    for deg in (-15.0, 0.0, 15.0):
        a = np.deg2rad(deg)
        eye = dist * np.array([np.sin(a), 0.0, np.cos(a)])
        E = np.eye(4)
        E[:3, :3] = np.stack([[np.cos(a), 0.0, -np.sin(a)], [0.0, -1.0, 0.0], -eye / dist])
        E[:3, 3] = -E[:3, :3] @ eye
        cams.append((K, E.astype(np.float32)))
        masks.append((((xs - W / 2) ** 2 + (ys - H / 2) ** 2) <= 560 ** 2).astype(np.uint8) * 255)
    return cams, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=280, help="sphere radius in voxels (280: about 3 M faces)")
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    verts, faces = sphere_mesh(a.radius)
    cams, masks = scene(a.radius * VOXEL)
    CM.clean_mesh(verts[:300], faces[:0], cams, [m[:48, :64] for m in masks])            # warm: library, allocator
    torch.cuda.synchronize()
    ops.profile_enable(True)
    t0 = time.perf_counter()
    v, f, st = CM.clean_mesh(verts, faces, cams, masks, return_stages=True)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    prof = ops.profile_read()
    ops.profile_enable(False)
    ms = lambda *names: sum(prof[n]["ms"] for n in names if n in prof)   # noqa: E731
    res = dict(mesh=f"sphere TSDF, {VOXEL} mm voxels, radius {a.radius} voxels", image="1200x1600", views=3,
               vertices=len(verts), faces=len(faces), faces_after_votes=len(st["faces2"]), faces_first_hit=len(st["faces3"]),
               faces_final=len(f), rays=int(sum((fid >= 0).sum() for fid in st["face_ids"])), component_rounds=st["rounds"],
               dilate_ms=ms("mask_dilate"), votes_ms=ms("mesh_vertex_votes"), first_hit_ms=ms("mesh_first_hit"),
               components_ms=ms("mesh_edge_keys", "mesh_mark_pairs", "mesh_component_round", "mesh_component_labels"),
               component_rounds_ms=ms("mesh_component_round"), end_to_end_ms=wall_ms)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
