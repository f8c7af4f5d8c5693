"""Benchmark of the mesh fly-through (uforecon_amd/render_trajectory.py) on a DTU-sized case: the marching-cubes mesh of a
synthetic sphere TSDF at 1.5 mm voxels (about 3 M faces), 240 frames of 640 x 800 along a path through three cameras on an arc
(the first key is also the last, as in the reference's [23, 24, 23]), smooth shading on a black background (a lit pixel is
at least 64, so the non-black share is the share of rays that hit), at supersample 1 and 2.
  * kernels: HIP events around every launch (ufr_profile_*), per frame -- first hit (the key-image reset, both triangle
    kernels and the resolve), shade, downsample -- and the vertex normals once;
  * end to end: ``render_mesh`` wall time, which adds the upload of the mesh, torch's sort for the vertex normals, the chunking
    and the copy of the frames to the host.
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
from bench_clean_mesh import VOXEL, sphere_mesh  # noqa: E402
from uforecon_amd import ops, render_trajectory as RT  # noqa: E402

H, W, FRAMES = 640, 800, 240


def key_cameras(radius_mm, focal=1450.0):
    dist = focal * radius_mm / 250.0                          # the sphere's image is about 250 pixels in radius
    K = np.array([[focal, 0, W / 2 + 0.37], [0, focal, H / 2 + 0.21], [0, 0, 1]], np.float32)
    w2cs = []
    for deg in (-15.0, 15.0, -15.0):
        a = np.deg2rad(deg)
        eye = dist * np.array([np.sin(a), 0.0, np.cos(a)])
        E = np.eye(4)
        E[:3, :3] = np.stack([[np.cos(a), 0.0, -np.sin(a)], [0.0, -1.0, 0.0], -eye / dist])
        E[:3, 3] = -E[:3, :3] @ eye
        w2cs.append(E)
    return K, np.stack(w2cs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=280, help="sphere radius in voxels (280: about 3 M faces)")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    verts, faces = sphere_mesh(a.radius)
    K, w2cs = key_cameras(a.radius * VOXEL)
    c2ws = RT.interpolate_trajectory(w2cs, a.frames)
    RT.render_mesh(verts[:300], faces[:0], K, c2ws[:1], 48, 64)                           # warm: library, allocator
    RT.render_mesh(verts, faces, K, c2ws[:2], H, W, supersample=2)
    torch.cuda.synchronize()
    res = dict(mesh=f"sphere TSDF, {VOXEL} mm voxels, radius {a.radius} voxels", image=f"{H}x{W}", frames=a.frames,
               vertices=len(verts), faces=len(faces))
    for s in (1, 2):
        ops.profile_enable(True)
        t0 = time.perf_counter()
        images = RT.render_mesh(verts, faces, K, c2ws, H, W, supersample=s, background=(0, 0, 0))
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        prof = ops.profile_read()
        ops.profile_enable(False)
        ms = lambda name: prof[name]["ms"] if name in prof else 0.0   # noqa: E731
        res[f"s{s}"] = dict(render=f"{s * H}x{s * W}", hit_pixel_share=float((images != 0).any(-1).mean()),
                            vertex_normals_ms=ms("raster_vertex_normals"), first_hit_ms_per_frame=ms("raster_first_hit") / a.frames,
                            shade_ms_per_frame=ms("raster_shade") / a.frames,
                            downsample_ms_per_frame=ms("raster_downsample") / a.frames,
                            end_to_end_ms=wall_ms, end_to_end_ms_per_frame=wall_ms / a.frames)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
