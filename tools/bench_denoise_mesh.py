"""Benchmark of mesh denoising (uforecon_amd/denoise_mesh.py, csrc/mesh_denoise.hip): the marching-cubes sphere of about 2 M
vertices of the other mesh benchmarks, the defaults (5 normal steps, 10 vertex steps, sigma_s the mean edge length, sigma_r
0.35).  Medians of 5 after a warm-up:
  * every kernel through HIP events around every launch (ufr_profile_*), in runs of their own;
  * ``ops.mesh_denoise`` end to end by wall clock (the sort of the corner slots and the index check included), ended by a
    device synchronise;
  * the bytes one normal step and one vertex step need -- every array a step reads or writes counted once, the gathered
    records, positions and normals as one read of their array -- and the TB/s that makes, beside the streaming-copy figure of
    about 6.3 TB/s; also the bytes the step's loads ask for when no gather hits a cache;
  * the same rule as torch float64 operations on the same device (``index_add_``: its sums are unordered, so only the largest
    difference is reported, for scale; it takes the border from the library's result);
  * ``ops.mesh_smooth``'s 10 Taubin iterations with cotangent weights on the same mesh, end to end.
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
from uforecon_amd import ops  # noqa: E402
from uforecon_amd.denoise_mesh import SIGMA_R, mean_edge_length  # noqa: E402

RUNS = 5
NORMAL_ITERATIONS = 5
VERTEX_ITERATIONS = 10
STREAM_COPY_TBS = 6.3
KERNELS = ("mesh_denoise_faces", "mesh_denoise_rows", "mesh_denoise_border", "mesh_denoise_normals", "mesh_denoise_vertices")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def _k(u):
    x = (1.0 - u / 256.0).clamp_min(0.0)
    for _ in range(8):
        x = x * x
    return x


def torch_same_rule(tv, tf, border, sigma_s, sigma_r, n_normal, n_vertex):
    """the rule of include/ufr.h as torch float64 operations, border fixed; unordered sums"""
    V, F = len(tv), len(tf)
    f = tf.long()
    p0, p1, p2 = tv[f[:, 0]], tv[f[:, 1]], tv[f[:, 2]]
    m = torch.linalg.cross(p1 - p0, p2 - p0)
    nf = m.norm(dim=1)
    live = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]) & (nf > 0) & torch.isfinite(nf)
    n = torch.where(live[:, None], m / nf.clamp_min(1e-300)[:, None], torch.zeros_like(m))
    A = torch.where(live, 0.5 * nf, torch.zeros_like(nf))
    c = (p0 + p1 + p2) / 3.0
    # the pairs (f, g) of live faces that share a vertex, each once: a self-join of the (vertex, face) rows on the vertex
    lf = torch.nonzero(live)[:, 0]
    rv, rg = f[lf].reshape(-1), lf.repeat_interleave(3)
    order = torch.argsort(rv, stable=True)
    rv, rg = rv[order], rg[order]
    start = torch.searchsorted(rv, torch.arange(V + 1, device=tv.device))
    deg = start[1:] - start[:-1]
    D = int(deg.max())
    table = torch.full((V, D), -1, dtype=torch.int64, device=tv.device)
    table[rv, torch.arange(len(rv), device=tv.device) - start[rv]] = rg
    a, b = table[:, :, None].expand(V, D, D), table[:, None, :].expand(V, D, D)
    ok = (a >= 0) & (b >= 0) & (a != b)
    pair = torch.unique(a[ok] * F + b[ok])
    pf, pg = pair // F, pair % F
    two_ss, two_rr = 2.0 * (sigma_s * sigma_s), 2.0 * (sigma_r * sigma_r)
    ws = A[pg] * _k(((c[pg] - c[pf]) ** 2).sum(1) / two_ss)
    for _ in range(n_normal):
        w = ws * _k(((n[pg] - n[pf]) ** 2).sum(1) / two_rr)
        acc = (A[:, None] * n).index_add_(0, pf, w[:, None] * n[pg])
        L = acc.norm(dim=1)
        good = live & (L > 0) & torch.isfinite(L)
        n = torch.where(good[:, None], acc / L.clamp_min(1e-300)[:, None], n)
    cnt = torch.zeros(V, dtype=torch.float64, device=tv.device).index_add_(0, rv, torch.ones(len(rv), dtype=torch.float64, device=tv.device))
    move = (cnt > 0) & (border == 0)
    safe = torch.where(move, cnt, torch.ones_like(cnt))[:, None]
    q = tv
    for _ in range(n_vertex):
        cg = (q[f[rg, 0]] + q[f[rg, 1]] + q[f[rg, 2]]) / 3.0
        d = ((cg - q[rv]) * n[rg]).sum(1)
        s = torch.zeros_like(q).index_add_(0, rv, n[rg] * d[:, None])
        q = torch.where(move[:, None], q + s / safe, q)
    return q, n, len(pair)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm (320: a mesh of about 2 M vertices)")
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    verts, faces = sphere_mesh(a.radius)
    faces = faces.astype(np.int32)
    dev = torch.device("cuda")
    tv, tf = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    V, F = len(verts), len(faces)
    sigma_s = mean_edge_length(verts, faces)
    kw = dict(normal_iterations=NORMAL_ITERATIONS, vertex_iterations=VERTEX_ITERATIONS, sigma_s=sigma_s, sigma_r=SIGMA_R)
    ops.mesh_denoise(tv, tf[:4096].contiguous(), 1, 1, sigma_s=sigma_s)                            # warm: library, allocator
    out = ops.mesh_denoise(tv, tf, **kw)                                                           # warm at this size
    r = dict(mesh=f"{V} vertices, {F} faces, a sphere of {a.radius * VOXEL} mm", runs=RUNS, statistic="median",
             normal_iterations=NORMAL_ITERATIONS, vertex_iterations=VERTEX_ITERATIONS, sigma_s_mm=sigma_s, sigma_r=SIGMA_R,
             stream_copy_tb_per_s=STREAM_COPY_TBS)
    r["end_to_end_ms"] = statistics.median(timed(lambda: ops.mesh_denoise(tv, tf, **kw))[1] for _ in range(RUNS))
    kern = {k: [] for k in KERNELS}
    for _ in range(RUNS):
        ops.profile_enable(True)
        ops.mesh_denoise(tv, tf, **kw)
        torch.cuda.synchronize()
        prof = ops.profile_read()
        ops.profile_enable(False)
        assert prof["mesh_denoise_normals"]["launches"] == NORMAL_ITERATIONS and prof["mesh_denoise_vertices"]["launches"] == VERTEX_ITERATIONS, prof
        for k in kern:
            kern[k].append(prof[k]["ms"] / prof[k]["launches"])
    r["kernel_ms"] = {k: statistics.median(x) for k, x in kern.items()}
    r["kernels_total_ms"] = (r["kernel_ms"]["mesh_denoise_faces"] + r["kernel_ms"]["mesh_denoise_rows"] + r["kernel_ms"]["mesh_denoise_border"]
                             + NORMAL_ITERATIONS * r["kernel_ms"]["mesh_denoise_normals"] + VERTEX_ITERATIONS * r["kernel_ms"]["mesh_denoise_vertices"])
    rows = int((out["normals"].abs().sum(1) > 0).sum()) * 3   # the live rows
    steps = {}
    # a normal step: the records in and out (64 bytes each), the corner indices, the rows' faces (4 bytes each), the run starts
    once = F * (64 + 64 + 12) + 3 * F * 4 + (V + 1) * 8
    steps["normals"] = dict(bytes=once)
    # a vertex step: positions in and out, run starts, border flags, the rows, the normals
    steps["vertices"] = dict(bytes=V * (24 + 24 + 8 + 1) + 3 * F * 16 + F * 24, bytes_without_cache=V * (24 + 24 + 8 + 1) + rows * (16 + 48 + 24))
    for name, key in (("normals", "mesh_denoise_normals"), ("vertices", "mesh_denoise_vertices")):
        steps[name]["tb_per_s"] = steps[name]["bytes"] / (r["kernel_ms"][key] * 1e-3) / 1e12
        steps[name]["share_of_stream_copy"] = steps[name]["tb_per_s"] / STREAM_COPY_TBS
    torch_same_rule(tv, tf, out["border"], sigma_s, SIGMA_R, NORMAL_ITERATIONS, VERTEX_ITERATIONS)      # warm
    runs = [timed(lambda: torch_same_rule(tv, tf, out["border"], sigma_s, SIGMA_R, NORMAL_ITERATIONS, VERTEX_ITERATIONS)) for _ in range(RUNS)]
    t_ms = statistics.median(ms for _, ms in runs)
    tq, tn, n_pairs = runs[0][0]
    # ... and were nothing cached: the run starts of three corners, every row of those runs, the indices of the second and
    # third corner's rows (two thirds of all), a record a neighbour
    deg = torch.bincount(tf.reshape(-1).long(), minlength=V)
    steps["normals"]["bytes_without_cache"] = F * (64 + 64 + 12 + 48) + int((deg * deg).sum()) * (4 + 8) + n_pairs * 64
    steps["normals"]["neighbours_per_face"] = n_pairs / max(rows // 3, 1)
    r["steps"] = steps
    r["torch_same_rule"] = dict(ms=t_ms, times_the_call=t_ms / r["end_to_end_ms"],
                                max_abs_difference_mm=float((tq - out["verts"]).abs().max()),
                                max_abs_normal_difference=float((tn - out["normals"]).abs().max()))
    del runs, tq, tn
    ops.mesh_smooth(tv, tf, iterations=10)                                                         # warm
    r["mesh_smooth_taubin_10_end_to_end_ms"] = statistics.median(timed(lambda: ops.mesh_smooth(tv, tf, iterations=10))[1] for _ in range(RUNS))
    moved = (out["verts"] - tv).norm(dim=1)
    rad_in, rad = tv.norm(dim=1), out["verts"].norm(dim=1)
    own = ops.mesh_denoise(tv, tf, 0, 0, sigma_s=sigma_s)["normals"]
    turn = torch.rad2deg(torch.acos((own * out["normals"]).sum(1).clamp(-1.0, 1.0)))
    r.update(border_vertices=int(out["border"].sum()), mean_displacement_mm=float(moved.mean()), max_displacement_mm=float(moved.max()),
             radial_rms_in_mm=float(rad_in.std()), radial_rms_out_mm=float(rad.std()), mean_radius_in_mm=float(rad_in.mean()),
             mean_radius_out_mm=float(rad.mean()), mean_normal_turn_deg=float(turn.mean()))
    again = ops.mesh_denoise(tv, tf, **kw)
    r["rerun_equals_bit_for_bit"] = bool(torch.equal(again["verts"], out["verts"]) and torch.equal(again["normals"], out["normals"]))
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
