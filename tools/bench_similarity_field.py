"""Benchmark of the similarity field: 512^3 voxels over the +-1 cube, 3 source views, match maps 128x160 (a 512x640 frame).
Each figure is one run on the device named in the result:
  * kernel: `ufr_similarity_field` (HIP events around the call, best of --reps), with and without the n_vis output, and the
    rate against the bytes it REQUESTS -- pairs x 2 sides x 4 taps x 128 B per voxel (arithmetic, not a measurement: the maps
    are 5 MB per view and stay cache resident);
  * the route there was before it: `ops.project_gather` with its sim8 output over the same points, grid columns as rays, in
    chunks below its point limit (its code is unchanged, so this is what the field cost before), HIP events over all chunks;
  * the oracle's torch expression (`project` + `pair_similarity`) on the device in the reference's 64^3 blocks;
  * marching cubes at 0.99 and at the field's median (at 0.99 a synthetic frame's field has no crossing), `field_mesh`;
  * `UFOReconInference.extract_similarity` end to end (encoder, field, mesh, PLY file), wall time.
Prints one JSON object; --out writes it to a file."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import load_weights  # noqa: E402
from oracle import ufo_oracle as O  # noqa: E402
from uforecon_amd import ops, pipeline  # noqa: E402
from uforecon_amd import similarity_field as SF  # noqa: E402
from uforecon_amd.scene import fill_state_dict, make_frame  # noqa: E402

DEV = "cuda:0"
LO, HI = [-1.0] * 3, [1.0] * 3


def _event_ms(fn, reps=1):
    best, out = float("inf"), None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best, out


def _wall_ms(fn, reps=1):
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def gather_route(fh, weights, tabs, rays_per_chunk):
    """The field through ufr_project_gather: columns of the grid as rays along z, sim8 averaged over its 8 columns."""
    gx, gy, gz = (t.to(DEV) for t in tabs)
    X, Y, Z = gx.numel(), gy.numel(), gz.numel()
    NV = fh.NV
    u = torch.empty(X * Y, Z, device=DEV)
    xx, yy = torch.meshgrid(gx, gy, indexing="ij")
    o_all = torch.stack([xx, yy, torch.zeros_like(xx)], -1).reshape(-1, 3).contiguous()
    d = torch.tensor([0., 0., 1.], device=DEV).expand(rays_per_chunk, 3).contiguous()
    z = gz[None].expand(rays_per_chunk, -1).contiguous()
    P = rays_per_chunk * Z
    out = (torch.empty(P, NV, 80, device=DEV), torch.empty(P, NV, 4, device=DEV), torch.empty(P, NV, 4, device=DEV))
    sim8 = torch.empty(P, 8, device=DEV)

    def run():
        for r0 in range(0, X * Y, rays_per_chunk):
            ops.project_gather(fh, weights, o_all[r0:r0 + rays_per_chunk], d, z, sim8_out=sim8, out=out)
            u[r0:r0 + rays_per_chunk] = sim8.view(rays_per_chunk, Z, 8).mean(-1)
        return u.view(X, Y, Z)

    return run


def oracle_route(frame_dev, tabs, block=64):
    """model.py:891-911 with the oracle's expressions on the device: 64^3 blocks, meshgrid, project, pair_similarity, mean."""
    poses = frame_dev.batch["source_poses"][0]
    match = frame_dev.match_feature[0][0]
    NV = poses.shape[0]
    tx, ty, tz = (t.to(DEV).split(block) for t in tabs)
    n = [sum(len(c) for c in t) for t in (tx, ty, tz)]
    u = torch.empty(*n, device=DEV)

    def run():
        with torch.no_grad():
            for xi, xs in enumerate(tx):
                for yi, ys in enumerate(ty):
                    for zi, zs in enumerate(tz):
                        pts = torch.stack(torch.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 1, 3)
                        xy, _, _ = O.project(poses, pts)
                        s = O.pair_similarity(xy, match, NV).mean(-1)
                        u[xi * block:xi * block + len(xs), yi * block:yi * block + len(ys), zi * block:zi * block + len(zs)] = \
                            s.reshape(len(xs), len(ys), len(zs))
        return u

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    R, NV, H, W = a.resolution, 3, 512, 640
    res = dict(resolution=R, voxels=R ** 3, source_views=NV, match_maps="%dx%d" % (H // 4, W // 4), device=torch.cuda.get_device_name(0),
               arch=torch.cuda.get_device_properties(0).gcnArchName,
               note="one run on the device named here; requested_bytes is arithmetic, not a measurement")
    fr = make_frame(H, W, NV, seed=5)
    f = fr.to(DEV)
    fh = ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)
    tabs = ops.grid_tables(LO, HI, R)
    ops.similarity_field(fh, LO, HI, 16)                                                   # warm: library, allocator
    # ---- the kernel
    u = torch.empty(R, R, R, device=DEV)
    n_vis = torch.empty(R, R, R, dtype=torch.uint8, device=DEV)
    import ctypes as C
    from uforecon_amd import _lib
    lib = _lib.load()
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    dim = (C.c_int32 * 3)(R, R, R)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    call = lambda nv: _lib.check(lib.ufr_similarity_field(C.byref(fh.frame), fp(tabs[0]), fp(tabs[1]), fp(tabs[2]), dim, u.data_ptr(),  # noqa: E731
                                                          nv, 0, stream()), "ufr_similarity_field")
    call(None)
    res["kernel_ms"], _ = _event_ms(lambda: call(None), a.reps)
    res["kernel_with_n_vis_ms"], _ = _event_ms(lambda: call(n_vis.data_ptr()), a.reps)
    npair = NV * (NV - 1) // 2
    res["requested_bytes"] = R ** 3 * npair * 2 * 4 * 128
    res["requested_gbps"] = res["requested_bytes"] / res["kernel_ms"] / 1e6
    res["written_bytes"] = R ** 3 * 4
    res["voxels_per_us"] = R ** 3 / res["kernel_ms"] / 1e3
    res["fraction_above_0.99"] = float((u > 0.99).float().mean())
    res["field_min_median_max"] = [float(u.min()), float(u.median()), float(u.max())]
    # ---- the gather route (the path before this kernel)
    weights = ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})
    rays = max(1, min(R * R, (1 << 21) // R))
    while (R * R) % rays:
        rays -= 1
    route = gather_route(fh, weights, tabs, rays)
    route()
    res["gather_route_ms"], ug = _event_ms(route, 1)
    res["gather_route_chunks"] = R * R // rays
    res["gather_route_points_per_chunk"] = rays * R
    res["gather_route_max_abs_diff"] = float((ug - u).abs().max())
    res["gather_route_over_kernel"] = res["gather_route_ms"] / res["kernel_ms"]
    del ug, route
    torch.cuda.empty_cache()
    # ---- the oracle's torch expression on the device
    orc = oracle_route(f, tabs)
    res["oracle_torch_blocks_ms"], uo = _event_ms(orc, 1)
    res["oracle_torch_max_abs_diff"] = float((uo - u).abs().max())
    res["oracle_torch_over_kernel"] = res["oracle_torch_blocks_ms"] / res["kernel_ms"]
    del uo
    torch.cuda.empty_cache()
    # ---- marching cubes
    level = float(u.median())
    ops.marching_cubes(-u, -0.99)
    res["marching_cubes_0.99_ms"], m = _wall_ms(lambda: ops.marching_cubes(-u, -0.99), a.reps)
    res["mesh_0.99_V_F"] = [int(m[0].shape[0]), int(m[1].shape[0])]
    res["median_level"] = level
    try:
        res["field_mesh_median_ms"], m = _wall_ms(lambda: SF.field_mesh(u, LO, HI, level), 1)
        res["mesh_median_V_F"] = [int(m[0].shape[0]), int(m[1].shape[0])]
    except (ops.UfrError, torch.cuda.OutOfMemoryError) as e:    # a synthetic field crosses its median everywhere
        res["field_mesh_median_error"] = str(e)[:200]
    m = None
    torch.cuda.empty_cache()
    # ---- end to end
    batch = f.batch
    pm = {}
    for st, s in (("stage1", 4), ("stage2", 2), ("stage3", 1)):
        p = torch.zeros(1, NV, 2, 4, 4, device=DEV)
        p[0, :, 0] = batch["w2cs"][0, :NV]
        K = batch["intrinsics"][0, :NV].clone()
        K[:, :2] = K[:, :2] / s
        p[0, :, 1, :3, :3] = K
        p[0, :, 1, 3, 3] = 1.0
        pm[st] = p
    batch["proj_matrices"] = pm
    near, far = float(batch["near_fars"][0, 0, 0]), float(batch["near_fars"][0, 0, 1])
    batch["depth_values_org_scale"] = torch.linspace(near, far, 48, device=DEV)[None]
    batch["meta"] = ["dtu-scan24-3-00000000"]
    args = argparse.Namespace(extract_geometry=True, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64, fine_sample=64,
                              volume_type="correlation", volume_reso=96, mvs_depth_guide=1, depth_pos_encoding=True, use_dir_srdf=False,
                              explicit_similarity=True, test_coarse_only=False, test_ray_num=800, test_n_view=3, out_dir=None)
    net = fill_state_dict(pipeline.UFOReconInference(args), 21).eval().to(DEV)
    net.load_state_dict(load_weights(), strict=False)
    with tempfile.TemporaryDirectory() as tmp:
        ue = net.extract_similarity(batch, resolution=R, out_dir=tmp)                      # warm: convolution search
        # the encoder runs on filled (untrained) weights: what its field looks like is recorded, not judged
        res["extract_similarity_fraction_above_0.99"] = float((ue > 0.99).float().mean())
        del ue
        res["extract_similarity_0.99_ms"], _ = _wall_ms(lambda: net.extract_similarity(batch, resolution=R, out_dir=tmp), 1)
        res["encode_frame_ms"], _ = _wall_ms(lambda: net.encode_frame(batch), 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
