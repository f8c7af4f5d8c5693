"""Micro-benchmark of marching cubes (csrc/mcubes.hip) on the fused wall scene of tools/bench_tsdf.py (384^3 = 56.6 M
voxels, 226 MB per volume): volume dims, V and F, per-kernel time from ufr_profile_* after warm-up, algorithmic bytes
and the HBM roofline fraction, end-to-end TSDFVolume.get_mesh() time, and -- for comparison -- the time of the
get_volume() copy that the scikit-image path needs before it can start.

Algorithmic bytes (what a kernel cannot avoid moving): count, verts and faces each read the volume once (4 B per voxel);
verts writes 24 B per vertex + 4 B of index per vertex-owning voxel; faces reads those index words and writes 12 B per
face; the scan's traffic is negligible.  hbm_frac = algorithmic bytes / kernel time / 8 TB/s (the figure bench_tsdf.py
uses)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_tsdf import scene  # noqa: E402
from uforecon_amd import ops, tsdf  # noqa: E402

KERNELS = ("mcubes_count", "mcubes_scan", "mcubes_verts", "mcubes_faces")


def _wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def measure(n: int = 384, reps: int = 10, verbose: bool = False):
    K, P, depth, bnds, vs = scene(n)
    vol = tsdf.TSDFVolume(bnds.copy(), voxel_size=vs, margin=3, integrate_color=True)
    d = torch.from_numpy(depth).cuda()
    vol.integrate(None, d, K, P)
    t = vol._tsdf_vol_gpu
    verts, faces, _ = ops.marching_cubes(t)           # warm-up (code objects, allocator)
    vol.get_mesh()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    torch.cuda.synchronize()
    ops.profile_enable(True)
    ops.profile_read()
    for _ in range(reps):
        ops.marching_cubes(t)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    ms = {k: prof[k]["ms"] / prof[k]["launches"] for k in KERNELS}
    n_vox = int(np.prod(vol._vol_dim))
    below = t < 0                                         # voxels that own a vertex (4 B of index each)
    own = torch.zeros_like(below)
    own[:-1] |= below[:-1] != below[1:]
    own[:, :-1] |= below[:, :-1] != below[:, 1:]
    own[:, :, :-1] |= below[:, :, :-1] != below[:, :, 1:]
    owners = int(own.sum())
    del below, own
    algo = {"mcubes_count": 4 * n_vox, "mcubes_scan": 0, "mcubes_verts": 4 * n_vox + 24 * V + 4 * owners,
            "mcubes_faces": 4 * n_vox + 12 * F + 12 * F}
    total_ms = sum(ms.values())
    total_algo = sum(algo.values())
    mc_ms = _wall_ms(lambda: ops.marching_cubes(t), reps)
    mesh_ms = _wall_ms(vol.get_mesh, reps)
    copy_ms = _wall_ms(vol.get_volume, max(2, reps // 3))
    res = dict(volume=[int(v) for v in vol._vol_dim], voxels=n_vox, V=V, F=F, owner_voxels=owners,
               kernel_ms={k: round(v, 4) for k, v in ms.items()}, kernels_ms=total_ms,
               algorithmic_bytes=total_algo, achieved_gbps=total_algo / total_ms / 1e6,
               hbm_frac=total_algo / total_ms / 1e6 / 8000,
               hbm_frac_per_kernel={k: (algo[k] / ms[k] / 1e6 / 8000 if algo[k] else None) for k in KERNELS},
               marching_cubes_ms=mc_ms, get_mesh_ms=mesh_ms, get_volume_copy_ms=copy_ms)
    if verbose:
        print(f"volume {tuple(vol._vol_dim)} = {n_vox / 1e6:.1f} M voxels: V {V}, F {F} ({owners} vertex-owning voxels)")
        for k in KERNELS:
            fr = res["hbm_frac_per_kernel"][k]
            print(f"  {k:13s} {ms[k] * 1e3:8.1f} us" + (f"   {algo[k] / 1e6:7.1f} MB  {fr:.1%} of 8 TB/s" if fr else ""))
        print(f"  kernels      {total_ms * 1e3:8.1f} us   {total_algo / 1e6:7.1f} MB  {res['hbm_frac']:.1%} of 8 TB/s")
        print(f"ops.marching_cubes {mc_ms:.3f} ms, get_mesh() {mesh_ms:.3f} ms end to end; get_volume() copy alone "
              f"{copy_ms:.3f} ms")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", help="also write the result as JSON to this path")
    a = ap.parse_args()
    res = measure(a.n, a.reps, verbose=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
