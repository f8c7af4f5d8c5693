"""Benchmark of mesh texturing (uforecon_amd/texture_mesh.py, csrc/mesh_texture.hip): bench_color_mesh's marching-cubes sphere
of about 2 M vertices simplified to about a tenth of them, its 49 synthetic 1200 x 1600 pictures from a ring of cameras, and the
default atlas (the largest patch size that fits 4096 x 4096).
  * stages: ``texture_mesh``'s own wall-clock milliseconds per stage (upload, the 49 depth maps, the vertex-colour fallback, the
    bake, the fill), each ended by a device synchronise, and the call end to end: medians of ``--runs`` calls after a warm-up;
  * kernels: HIP events around every launch (ufr_profile_*) in a run of its own;
  * the same rule as torch float64 operations on the same device, view by view over all texels of a face (bench_color_mesh's
    ``one_view`` on the texels' points and face normals; the bytes are compared and reported, not asserted);
  * the same rule in vectorised numpy on the host for ONE view, for scale;
  * the bytes the bake needs -- a face's indices, corners and fallback colours once, four depths per (texel, view) pair that
    reaches the depth test, twelve picture bytes per pair that passes it, four bytes out per texel -- over its kernel time,
    beside the 6.3 TB/s a streaming copy reaches on this device.
Nothing earlier exists to compare with, so no threshold is set.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_clean_mesh import VOXEL, sphere_mesh  # noqa: E402
from bench_color_mesh import H, VIEWS, W, one_view, ring_cameras  # noqa: E402
from uforecon_amd import color_mesh as CMesh, ops, texture_mesh as TM, texture_ops as TO  # noqa: E402

STREAM_BYTES_PER_SECOND = 6.3e12


def texel_points(verts, faces, S, xp, dev=None):
    """(keep (Ht,Wt) bool, p (T,3), n (T,3)): the texels that belong to a face, and their points and unit face normals in
    row-major order over the atlas, by the closed form of include/ufr.h"""
    F = len(faces)
    Ht, Wt, cols, _ = TO.atlas_layout(F, S)
    C = S + 3
    ys, xs = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    i, j = xs % C, ys % C
    odd = i + j > S + 2
    face = 2 * ((ys // C) * cols + xs // C) + odd
    i, j = np.where(odd, C - 1 - i, i), np.where(odd, C - 1 - j, j)
    keep = face < F
    face, i, j = face[keep], i[keep], j[keep]
    wb, wc = i / float(S), j / float(S)
    wa = (1.0 - wb) - wc
    conv = (lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)) if xp is torch else (lambda t: t)
    fa = conv(faces[face].astype(np.int64))
    v = conv(verts)
    wa, wb, wc = conv(wa)[:, None], conv(wb)[:, None], conv(wc)[:, None]
    a, b, c = v[fa[:, 0]], v[fa[:, 1]], v[fa[:, 2]]
    p = (wa * a + wb * b) + wc * c
    u, w = b - a, c - a
    n = xp.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    ln = xp.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    n = n / ln[:, None]
    return keep, p, n


def torch_bake(p, n, ti, td, k, w2c, centre, z_min, depth_tol, min_cos, power):
    dev = p.device
    A = torch.zeros((len(p), 3), dtype=torch.float64, device=dev)
    Ws = torch.zeros(len(p), dtype=torch.float64, device=dev)
    used = torch.zeros(len(p), dtype=torch.int32, device=dev)
    reached_pairs = 0
    for i in range(len(k)):
        ok, w, s, reached = one_view(torch, p, n, ti[i], td[i], torch.from_numpy(k[i]).to(dev), torch.from_numpy(w2c[i]).to(dev),
                                     torch.from_numpy(centre[i]).to(dev), z_min, 1.0 + depth_tol, min_cos, power)
        A = A + torch.where(ok[:, None], w[:, None] * s, torch.zeros_like(s))
        Ws = Ws + torch.where(ok, w, torch.zeros_like(w))
        used = used + ok.to(torch.int32)
        reached_pairs = reached_pairs + reached.sum()
    col = torch.clamp(torch.nan_to_num(torch.round(A / Ws[:, None]), nan=0.0), 0, 255).to(torch.uint8)
    return col, used.to(torch.uint8), int(reached_pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm (320: a mesh of about 2 M vertices)")
    ap.add_argument("--ratio", type=float, default=0.1, help="the share of the vertices the simplifier keeps")
    ap.add_argument("--views", type=int, default=VIEWS)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_texture_mesh: no GPU: nothing is measured without one")
    dev = torch.device("cuda")
    full_v, full_f = sphere_mesh(a.radius)
    simple = ops.mesh_simplify(torch.from_numpy(full_v).to(dev), torch.from_numpy(full_f.astype(np.int32)).to(dev),
                               target_vertices=int(np.ceil(a.ratio * len(full_v))))
    verts, faces = simple["verts"].cpu().numpy(), simple["faces"].cpu().numpy()
    cams = ring_cameras(a.views, a.radius * VOXEL)
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(a.views)]
    S = TO.patch_for_atlas(len(faces), TM.ATLAS_SIZE)
    Ht, Wt, _, _ = TO.atlas_layout(len(faces), S)
    TM.texture_mesh(verts, faces, cams[:2], images[:2])                                        # warm: library, allocator
    torch.cuda.synchronize()
    res = dict(mesh=f"{len(verts)} vertices, {len(faces)} faces: a sphere of {a.radius * VOXEL} mm with {len(full_v)} vertices, simplified",
               image=f"{H}x{W}", views=a.views, atlas=[Wt, Ht], patch=S, depth_tol=CMesh.DEPTH_TOL, min_cos=CMesh.MIN_COS,
               power=CMesh.POWER, fill_rounds=TM.FILL_ROUNDS, runs=a.runs)
    end, stages = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        tex, xy, used, state, ms = TM.texture_mesh(verts, faces, cams, images, return_timings=True)
        torch.cuda.synchronize()
        end.append((time.perf_counter() - t0) * 1e3)
        stages.append(ms)
    res["end_to_end_ms"] = statistics.median(end)
    res["stages"] = {k: statistics.median(m[k] for m in stages) for k in stages[0]}
    res["texels"] = {name: int(c) for name, c in zip(TM.STATE_NAMES, np.bincount(state.reshape(-1), minlength=5))}
    # kernels, in a run of their own
    ops.profile_enable(True)
    TM.texture_mesh(verts, faces, cams, images)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    res["kernels_ms"] = {k: dict(ms=v["ms"], launches=v["launches"]) for k, v in prof.items()}
    kernel_ms = prof["mesh_texture_bake"]["ms"]
    # the same rule as torch operations on the same device
    tv = torch.from_numpy(verts).to(dev)
    tf = torch.from_numpy(faces.astype(np.int32)).to(dev)
    ti = torch.from_numpy(np.stack(images)).to(dev)
    td = torch.empty((a.views, H, W), dtype=torch.float32, device=dev)
    for i, (K, E) in enumerate(cams):
        k_inv, c2w = CMesh.ray_camera(K, E)
        td[i] = ops.raster_frames(tv, tf, k_inv, c2w[None], H, W, return_depth=True, check_indices=False)["depth"][0]
    pk, pw, pc = (np.stack(x) for x in zip(*[CMesh.projection_camera(K, E) for K, E in cams]))
    args = (0.0, CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER)
    keep, p, n = texel_points(verts, faces, S, torch, dev)
    torch_bake(p, n, ti[:2], td[:2], pk[:2], pw[:2], pc[:2], *args)                                       # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep, p, n = texel_points(verts, faces, S, torch, dev)
    tcol, tused, reached = torch_bake(p, n, ti, td, pk, pw, pc, *args)
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) * 1e3
    gtex, gused = TO.mesh_texture_bake(tv, tf, ti, td, pk, pw, pc, S)
    tk = torch.from_numpy(keep).to(dev)
    gcol, gu = gtex[tk], gused[tk]
    seen = gu > 0
    res["torch_same_rule"] = dict(ms=torch_ms, times_the_kernel=torch_ms / kernel_ms, views_used_equal=bool(torch.equal(tused, gu)),
                                  colours_equal=bool(torch.equal(tcol[seen], gcol[seen])),
                                  max_level_difference=int((tcol[seen].int() - gcol[seen].int()).abs().max()))
    # bytes the kernel needs
    used_pairs = int(gu.sum(dtype=torch.int64))
    n_texels = int(keep.sum())
    need = len(faces) * (12 + 72) + Ht * Wt * 4 + reached * 16 + used_pairs * 12
    rate = need / (kernel_ms * 1e-3)
    res["bake_kernel"] = dict(ms=kernel_ms, texels=Ht * Wt, texels_of_a_face=n_texels, texel_view_pairs=n_texels * a.views,
                              pairs_at_the_depth_test=reached, pairs_sampled=used_pairs, bytes_needed=need,
                              achieved_gigabytes_per_second=rate / 1e9, streaming_copy_gigabytes_per_second=STREAM_BYTES_PER_SECOND / 1e9,
                              share_of_streaming_copy=rate / STREAM_BYTES_PER_SECOND, pairs_per_second=n_texels * a.views / (kernel_ms * 1e-3))
    # the numpy host form of one view
    hd = td[0].cpu().numpy()
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        _, hp, hn = texel_points(verts, faces, S, np)
        one_view(np, hp, hn, images[0], hd, pk[0], pw[0], pc[0], 0.0, 1.0 + CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER)
    res["numpy_one_view_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
