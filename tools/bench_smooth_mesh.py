"""Benchmark of mesh smoothing (uforecon_amd/smooth_mesh.py, csrc/mesh_smooth.hip): the marching-cubes sphere of about 2 M
vertices of the other mesh benchmarks, 10 Taubin iterations (20 steps) per weight mode.  Medians of 5 after a warm-up:
  * the rows and border kernels and one step, through HIP events around every launch (ufr_profile_*), in runs of their own;
  * ``ops.mesh_smooth`` end to end by wall clock (the sort of the corner slots and the index check included), ended by a
    device synchronise;
  * the bytes one step needs -- every array it reads or writes counted once, the gathered neighbour positions as the one read
    of the position array -- and the TB/s that makes, beside the streaming-copy figure of about 6.3 TB/s; also the bytes the
    step's loads ask for when no gather hits a cache;
  * the same rule as torch float64 ``index_add_`` operations on the same device: its sums are unordered, so only the largest
    difference is reported, for scale;
  * one step of the numpy statement (tests/smooth_ref.py) on the host.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_ref  # noqa: E402
from bench_clean_mesh import VOXEL, sphere_mesh  # noqa: E402
from uforecon_amd import ops  # noqa: E402

RUNS = 5
ITERATIONS = 10
STREAM_COPY_TBS = 6.3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def torch_same_rule(tv, tf, weights, factors):
    """the rule of include/ufr.h as torch float64 operations, border fixed; unordered sums"""
    V = len(tv)
    f = tf.long()
    live = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if weights == "cotangent":
        nf = torch.linalg.cross(tv[f[:, 1]] - tv[f[:, 0]], tv[f[:, 2]] - tv[f[:, 0]]).norm(dim=1)
        live &= (nf > 0) & torch.isfinite(nf)
    f = f[live]
    v = f.reshape(-1)
    a, b = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    if weights == "cotangent":
        nf3 = nf[live].repeat_interleave(3)
        wa = (((tv[v] - tv[b]) * (tv[a] - tv[b])).sum(1) / nf3).clamp(0.0, 64.0)
        wb = (((tv[v] - tv[a]) * (tv[b] - tv[a])).sum(1) / nf3).clamp(0.0, 64.0)
    else:
        wa = wb = torch.ones(len(v), dtype=torch.float64, device=tv.device)
    pair, count = torch.unique(torch.cat([v * V + a, v * V + b]), return_counts=True)
    held = torch.zeros(V, dtype=torch.bool, device=tv.device)
    held[pair[count != 2] // V] = True
    den = torch.zeros(V, dtype=torch.float64, device=tv.device).index_add_(0, v, wa + wb)
    move = (den > 0) & ~held
    safe = torch.where(move, den, torch.ones_like(den))[:, None]
    p = tv
    for t in factors:
        num = torch.zeros_like(p).index_add_(0, v, wa[:, None] * (p[a] - p[v]) + wb[:, None] * (p[b] - p[v]))
        p = torch.where(move[:, None], p + (t * num) / safe, p)
    return p


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
    steps = 2 * ITERATIONS
    factors = ops.smooth_factors("taubin", ITERATIONS)
    ops.mesh_smooth(tv, tf[:4096].contiguous(), iterations=1)                                      # warm: library, allocator
    res = dict(mesh=f"{V} vertices, {F} faces, a sphere of {a.radius * VOXEL} mm", runs=RUNS, statistic="median",
               method="taubin", iterations=ITERATIONS, steps=steps, stream_copy_tb_per_s=STREAM_COPY_TBS, weights={})
    for weights in ("cotangent", "uniform"):
        r = {}
        out = ops.mesh_smooth(tv, tf, weights=weights, iterations=ITERATIONS)                      # warm at this size
        r["end_to_end_ms"] = statistics.median(timed(lambda: ops.mesh_smooth(tv, tf, weights=weights, iterations=ITERATIONS))[1]
                                               for _ in range(RUNS))
        kern = {"mesh_smooth_rows": [], "mesh_smooth_border": [], "mesh_smooth_step": []}
        for _ in range(RUNS):
            ops.profile_enable(True)
            ops.mesh_smooth(tv, tf, weights=weights, iterations=ITERATIONS)
            torch.cuda.synchronize()
            prof = ops.profile_read()
            ops.profile_enable(False)
            assert prof["mesh_smooth_step"]["launches"] == steps, prof
            for k in kern:
                kern[k].append(prof[k]["ms"] / prof[k]["launches"])
        r["rows_kernel_ms"] = statistics.median(kern["mesh_smooth_rows"])
        r["border_kernel_ms"] = statistics.median(kern["mesh_smooth_border"])
        r["step_kernel_ms"] = statistics.median(kern["mesh_smooth_step"])
        row = 8 + (16 if weights == "cotangent" else 0)
        once = V * (24 + 24 + 8 + 1) + 3 * F * row            # positions in and out, run starts, border flags; the rows
        asked = once + 3 * F * 48                             # ... and two neighbour positions a row, were none of them cached
        r["step_bytes"] = once
        r["step_bytes_without_cache"] = asked
        r["step_tb_per_s"] = once / (r["step_kernel_ms"] * 1e-3) / 1e12
        r["step_share_of_stream_copy"] = r["step_tb_per_s"] / STREAM_COPY_TBS
        torch_same_rule(tv, tf, weights, factors)                                                  # warm
        runs = [timed(lambda: torch_same_rule(tv, tf, weights, factors)) for _ in range(RUNS)]
        t_ms = statistics.median(ms for _, ms in runs)
        r["torch_same_rule"] = dict(ms=t_ms, times_the_call=t_ms / r["end_to_end_ms"],
                                    max_abs_difference_mm=float((runs[0][0] - out["verts"]).abs().max()))
        moved = (out["verts"] - tv).norm(dim=1)
        rad = out["verts"].norm(dim=1)
        r.update(border_vertices=int(out["border"].sum()), mean_displacement_mm=float(moved.mean()),
                 max_displacement_mm=float(moved.max()), radial_rms_in_mm=float(tv.norm(dim=1).std()), radial_rms_out_mm=float(rad.std()),
                 mean_radius_in_mm=float(tv.norm(dim=1).mean()), mean_radius_out_mm=float(rad.mean()))
        rows = smooth_ref.rows(verts, faces, weights)
        held = smooth_ref.border_of(V, rows[0], rows[1], rows[2]) != 0
        t0 = time.perf_counter()
        first = smooth_ref.step(verts, factors[0], rows, held)
        r["numpy_one_step_ms"] = (time.perf_counter() - t0) * 1e3
        r["numpy_one_step_times_the_kernel"] = r["numpy_one_step_ms"] / r["step_kernel_ms"]
        one = ops.mesh_smooth(tv, tf, method="laplacian", weights=weights, iterations=1)["verts"].cpu().numpy()
        r["one_step_equals_numpy_bit_for_bit"] = bool(one.tobytes() == first.tobytes())
        res["weights"][weights] = r
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
