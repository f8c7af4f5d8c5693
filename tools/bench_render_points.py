"""Benchmark of the point-cloud fly-through (uforecon_amd/render_trajectory.py's render_points, csrc/splat.hip): a synthetic
cloud of 2 M coloured points on a sphere, 240 frames of 640 x 800 along bench_render_trajectory's path, radius 1, the default
eye-dome lighting, on a black background.
  * kernels: HIP events around every launch (ufr_profile_*), per frame -- splat (the key-image reset and the kernel) and resolve;
  * end to end: ``render_points`` wall time without the events, which adds the upload of the cloud, the chunking and the copy of
    the frames to the host;
  * the recorded references: the numpy restatement (tests/points_ref.py) of one frame on the host, and ``render_mesh`` of a
    marching-cubes sphere of comparable vertex count along the same path.
Nothing earlier exists to compare with, so no threshold is set.  Prints one JSON line; --out writes it to a file."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import points_ref as PR  # noqa: E402
from bench_clean_mesh import VOXEL, sphere_mesh  # noqa: E402
from bench_render_trajectory import FRAMES, H, W, key_cameras  # noqa: E402
from uforecon_amd import ops, render_trajectory as RT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm (320: a mesh of about 2 M vertices)")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--point_radius", type=int, default=1)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    d = rng.normal(size=(a.points, 3))
    pts = d / np.linalg.norm(d, axis=1, keepdims=True) * (a.radius * VOXEL)
    colors = rng.integers(0, 256, (a.points, 3)).astype(np.uint8)
    K, w2cs = key_cameras(a.radius * VOXEL)
    c2ws = RT.interpolate_trajectory(w2cs, a.frames)
    kw = dict(colors=colors, radius=a.point_radius, background=(0, 0, 0))
    RT.render_points(pts[:300], K, c2ws[:1], 48, 64)                                       # warm: library, allocator
    RT.render_points(pts, K, c2ws[:2], H, W, **kw)
    torch.cuda.synchronize()
    res = dict(cloud=f"{a.points} points on a sphere of {a.radius * VOXEL} mm, uint8 colours", image=f"{H}x{W}", frames=a.frames,
               point_radius=a.point_radius, edl_strength=RT.DEFAULT_EDL)
    t0 = time.perf_counter()
    images = RT.render_points(pts, K, c2ws, H, W, **kw)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    res.update(end_to_end_ms=wall_ms, end_to_end_ms_per_frame=wall_ms / a.frames,
               end_to_end_frames_per_second=a.frames / (wall_ms * 1e-3))
    ops.profile_enable(True)
    _, ids = RT.render_points(pts, K, c2ws, H, W, return_point_ids=True, **kw)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    res.update(covered_pixel_share=float((ids >= 0).mean()), splat_ms_per_frame=prof["splat"]["ms"] / a.frames,
               resolve_ms_per_frame=prof["splat_resolve"]["ms"] / a.frames)
    # reference 1: the numpy restatement of frame 0 on the host
    t0 = time.perf_counter()
    ref = PR.render(pts, PR.normalised_k(K), np.linalg.inv(c2ws[0]), H, W, colors=colors, radius=a.point_radius, background=(0, 0, 0),
                    edl_strength=RT.DEFAULT_EDL)
    res["numpy_restatement_ms_per_frame"] = (time.perf_counter() - t0) * 1e3
    res["frame0_ids_equal_restatement"] = bool(np.array_equal(ref["point_id"], ids[0]))
    res["frame0_image_max_level_difference"] = int(np.abs(ref["image"].astype(np.int32) - images[0].astype(np.int32)).max())
    # reference 2: the mesh renderer on a sphere of comparable vertex count, same path
    verts, faces = sphere_mesh(a.radius)
    RT.render_mesh(verts, faces, K, c2ws[:2], H, W)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    RT.render_mesh(verts, faces, K, c2ws, H, W, background=(0, 0, 0))
    torch.cuda.synchronize()
    mesh_ms = (time.perf_counter() - t0) * 1e3
    res["render_mesh"] = dict(vertices=len(verts), faces=len(faces), end_to_end_ms_per_frame=mesh_ms / a.frames,
                              end_to_end_frames_per_second=a.frames / (mesh_ms * 1e-3))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
