"""Benchmark of mesh colouring (uforecon_amd/color_mesh.py, csrc/mesh_color.hip): a marching-cubes sphere of about 2 M vertices
(bench_render_points' mesh) and 49 synthetic 1200 x 1600 pictures from a ring of cameras round it.
  * stages: ``color_mesh``'s own wall-clock milliseconds per stage (upload, normals, the 49 depth maps, the colour kernel, the
    fill), each ended by a device synchronise, and the call end to end;
  * kernels: HIP events around every launch (ufr_profile_*) in a run of its own;
  * the same rule as torch float64 operations on the same device, view by view (explicit gathers: ``grid_sample`` rounds
    differently and has no four-texel minimum; the bytes are compared and reported, not asserted);
  * the same rule in vectorised numpy on the host for ONE view, for scale;
  * the bytes the colour kernel needs -- the vertex and its normal once, four depths per (vertex, view) pair that reaches the
    depth test, twelve picture bytes per pair that passes it, four bytes out -- over its kernel time.
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
from bench_clean_mesh import VOXEL, sphere_mesh  # noqa: E402
from uforecon_amd import color_mesh as CMesh, ops  # noqa: E402

H, W, FOCAL, VIEWS = 1200, 1600, 2900.0, 49


def ring_cameras(n, radius_mm):
    """``n`` (K, E) float32 pairs on a ring round the y axis; the sphere's image is about 500 pixels in radius"""
    dist = FOCAL * radius_mm / 500.0
    K = np.array([[FOCAL, 0, W / 2 + 0.37], [0, FOCAL, H / 2 + 0.21], [0, 0, 1]], np.float32)
    cams = []
    for i in range(n):
        a = 2 * np.pi * i / n
        eye = dist * np.array([np.sin(a), 0.0, np.cos(a)])
        E = np.eye(4)
        E[:3, :3] = np.stack([[np.cos(a), 0.0, -np.sin(a)], [0.0, -1.0, 0.0], -eye / dist])
        E[:3, 3] = -E[:3, :3] @ eye
        cams.append((K, E.astype(np.float32)))
    return cams


def one_view(xp, v, nrm, img, dep, k, w2c, centre, z_min, one_tol, min_cos, power):
    """the rule of include/ufr.h for one view over all vertices, in ``xp`` = torch or numpy float64: (ok, w, s, reached) with
    ``reached`` the pairs that come as far as the depth test"""
    W_, H_ = img.shape[1], img.shape[0]
    px, py, pz = v[:, 0], v[:, 1], v[:, 2]
    c = [((w2c[i, 0] * px + w2c[i, 1] * py) + w2c[i, 2] * pz) + w2c[i, 3] for i in range(3)]
    ok = xp.isfinite(px) & xp.isfinite(py) & xp.isfinite(pz) & xp.isfinite(c[0]) & xp.isfinite(c[1]) & xp.isfinite(c[2]) & (c[2] > z_min)
    q = [(k[i, 0] * c[0] + k[i, 1] * c[1]) + k[i, 2] * c[2] for i in range(3)]
    x, y = q[0] / q[2], q[1] / q[2]
    xf, yf = xp.floor(x), xp.floor(y)
    ok = ok & (xf >= 0) & (xf + 1 <= W_ - 1) & (yf >= 0) & (yf + 1 <= H_ - 1)
    fx, fy = x - xf, y - yf
    e = [px - centre[0], py - centre[1], pz - centre[2]]
    ln = xp.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    cosv = xp.abs((nrm[:, 0] * (e[0] / ln) + nrm[:, 1] * (e[1] / ln)) + nrm[:, 2] * (e[2] / ln))
    ok = ok & (cosv >= min_cos) & (cosv > 0)
    reached = ok
    zero = xp.zeros_like(xf)
    base = xp.where(ok, yf, zero) * W_ + xp.where(ok, xf, zero)
    base = base.long() if xp is torch else base.astype(np.int64)
    d = dep.reshape(-1)
    D = [d[base], d[base + 1], d[base + W_], d[base + W_ + 1]]
    dmin = xp.minimum(xp.minimum(D[0], D[1]), xp.minimum(D[2], D[3]))
    dmin = dmin.double() if xp is torch else dmin.astype(np.float64)
    ok = ok & (D[0] > 0) & (D[1] > 0) & (D[2] > 0) & (D[3] > 0) & (c[2] <= one_tol * dmin)
    w = cosv * 0 + 1
    for _ in range(power):
        w = w * cosv
    im = img.reshape(-1, 3)
    cast = (lambda t: t.double()) if xp is torch else (lambda t: t.astype(np.float64))
    i00, i01, i10, i11 = cast(im[base]), cast(im[base + 1]), cast(im[base + W_]), cast(im[base + W_ + 1])
    gx, gy, fx, fy = (1.0 - fx)[:, None], (1.0 - fy)[:, None], fx[:, None], fy[:, None]
    s = gy * (gx * i00 + fx * i01) + fy * (gx * i10 + fx * i11)
    return ok, w, s, reached


def torch_colors(tv, tn, ti, td, k, w2c, centre, z_min, depth_tol, min_cos, power, fill):
    dev = tv.device
    A = torch.zeros((len(tv), 3), dtype=torch.float64, device=dev)
    Ws = torch.zeros(len(tv), dtype=torch.float64, device=dev)
    used = torch.zeros(len(tv), dtype=torch.int32, device=dev)
    reached_pairs = 0
    for i in range(len(k)):
        ok, w, s, reached = one_view(torch, tv, tn, ti[i], td[i], torch.from_numpy(k[i]).to(dev), torch.from_numpy(w2c[i]).to(dev),
                                     torch.from_numpy(centre[i]).to(dev), z_min, 1.0 + depth_tol, min_cos, power)
        A = A + torch.where(ok[:, None], w[:, None] * s, torch.zeros_like(s))
        Ws = Ws + torch.where(ok, w, torch.zeros_like(w))
        used = used + ok.to(torch.int32)
        reached_pairs = reached_pairs + reached.sum()
    col = torch.clamp(torch.nan_to_num(torch.round(A / Ws[:, None]), nan=0.0), 0, 255).to(torch.uint8)
    col = torch.where((used > 0)[:, None], col, torch.tensor(fill, dtype=torch.uint8, device=dev)[None])
    return col, used.to(torch.uint8), int(reached_pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm (320: a mesh of about 2 M vertices)")
    ap.add_argument("--views", type=int, default=VIEWS)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    verts, faces = sphere_mesh(a.radius)
    cams = ring_cameras(a.views, a.radius * VOXEL)
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(a.views)]
    CMesh.color_mesh(verts, faces, cams[:2], images[:2])                                       # warm: library, allocator
    torch.cuda.synchronize()
    res = dict(mesh=f"{len(verts)} vertices, {len(faces)} faces, a sphere of {a.radius * VOXEL} mm", image=f"{H}x{W}", views=a.views,
               depth_tol=CMesh.DEPTH_TOL, min_cos=CMesh.MIN_COS, power=CMesh.POWER, fill_rounds=CMesh.FILL_ROUNDS, runs=1)
    t0 = time.perf_counter()
    colors, used, state, ms = CMesh.color_mesh(verts, faces, cams, images, return_timings=True)
    torch.cuda.synchronize()
    res["end_to_end_ms"] = (time.perf_counter() - t0) * 1e3
    res["stages"] = ms
    res.update(seen=int((state == CMesh.STATE_SEEN).sum()), filled=int((state == CMesh.STATE_FILLED).sum()),
               empty=int((state == CMesh.STATE_EMPTY).sum()), views_used_histogram=np.bincount(used).tolist())
    # kernels, in a run of their own
    ops.profile_enable(True)
    CMesh.color_mesh(verts, faces, cams, images)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    res["kernels_ms"] = {k: dict(ms=v["ms"], launches=v["launches"]) for k, v in prof.items()}
    kernel_ms = prof["mesh_vertex_colors"]["ms"]
    # the same rule as torch operations on the same device
    dev = torch.device("cuda")
    tv = torch.from_numpy(verts).to(dev)
    tf = torch.from_numpy(faces.astype(np.int32)).to(dev)
    tn = ops.raster_vertex_normals(tv, tf)
    ti = torch.from_numpy(np.stack(images)).to(dev)
    td = torch.empty((a.views, H, W), dtype=torch.float32, device=dev)
    for i, (K, E) in enumerate(cams):
        k_inv, c2w = CMesh.ray_camera(K, E)
        td[i] = ops.raster_frames(tv, tf, k_inv, c2w[None], H, W, return_depth=True, check_indices=False)["depth"][0]
    pk, pw, pc = (np.stack(x) for x in zip(*[CMesh.projection_camera(K, E) for K, E in cams]))
    args = (0.0, CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER, CMesh.FILL_COLOR)
    torch_colors(tv, tn, ti[:2], td[:2], pk[:2], pw[:2], pc[:2], *args)                                  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tcol, tused, reached = torch_colors(tv, tn, ti, td, pk, pw, pc, *args)
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) * 1e3
    gcol, gused = ops.mesh_vertex_colors(tv, tn, ti, td, pk, pw, pc)
    res["torch_same_rule"] = dict(ms=torch_ms, times_the_kernel=torch_ms / kernel_ms, views_used_equal=bool(torch.equal(tused, gused)),
                                  colours_equal=bool(torch.equal(tcol, gcol)),
                                  max_level_difference=int((tcol.int() - gcol.int()).abs().max()))
    # bytes the kernel needs
    used_pairs = int(gused.sum(dtype=torch.int64))
    need = len(verts) * (24 + 24 + 4) + reached * 16 + used_pairs * 12
    res["colour_kernel"] = dict(ms=kernel_ms, vertex_view_pairs=len(verts) * a.views, pairs_at_the_depth_test=reached,
                                pairs_sampled=used_pairs, bytes_needed=need, achieved_bytes_per_second=need / (kernel_ms * 1e-3),
                                pairs_per_second=len(verts) * a.views / (kernel_ms * 1e-3))
    # the numpy host form of one view
    hn, hd = tn.cpu().numpy(), td[0].cpu().numpy()
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        one_view(np, verts, hn, images[0], hd, pk[0], pw[0], pc[0], 0.0, 1.0 + CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER)
    res["numpy_one_view_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
