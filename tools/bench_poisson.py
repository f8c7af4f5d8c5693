"""Benchmark of the Poisson reconstruction (uforecon_amd/poisson_mesh.py, csrc/poisson.hip) on the 2 M-point noisy sphere of
bench_pcd_filter.py (radius 480 mm, seed 0, radial noise 0.1 %), the exact outward directions as normals, at ``resolution``
128 and 256:
  * the wall time of every stage (grid, splat, divergence, solve, iso, marching cubes, density), each ending in a device
    synchronisation, the median and the range of ``--runs`` runs after one warm-up run;
  * the conjugate gradients: iterations, ms per iteration (the solve's time over its iterations: it includes the looks of
    the host) and the achieved bytes per second against the 88 bytes per node and iteration of the sketch (11 volume passes)
    and the 6.3 TB/s a streaming kernel reaches on the MI355X's HBM (8 TB/s on paper);
  * for comparison, the same three steps as torch fp64 operations on the same device for the same number of iterations
    (padded volume, slices, two .sum() reductions whose scalars stay on the device);
  * for scale only, ``scipy.sparse.linalg.cg`` on the host at resolution 128 with the matrix of tests/poisson_ref.py.
No threshold: nothing earlier exists to compare with.  No real scan and no trained checkpoint is involved.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import poisson_ref as R  # noqa: E402
from bench_clean_mesh import VOXEL  # noqa: E402
from uforecon_amd import ops  # noqa: E402

BYTES_PER_NODE = 88      # q = A p: 2 passes; x, r update: 6; p update: 3
HBM_MEASURED = 6.3e12    # bytes per second a streaming kernel reaches (8.0e12 on paper)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stages(p, n, resolution, pad, tol):
    """one reconstruction, stage by stage: (times in ms, facts)"""
    t = {}
    (origin, h, dims), t["grid"] = timed(lambda: ops.poisson_grid(p, resolution, pad))
    (V, W), t["splat"] = timed(lambda: ops.poisson_splat(p, n, origin, h, dims))
    b, t["divergence"] = timed(lambda: ops.poisson_divergence(V, h))
    del V
    ws = torch.empty(ops.poisson_workspace_bytes(dims), dtype=torch.uint8, device=p.device)
    (chi, info), t["solve"] = timed(lambda: ops.poisson_solve(b, h, tol, workspace=ws))
    (_, iso), t["iso"] = timed(lambda: ops.poisson_sample(chi, origin, h, p, return_mean=True))
    (v, f, _), t["marching_cubes"] = timed(lambda: ops.marching_cubes((chi - float(iso)).float(), 0.0))
    verts = (torch.tensor(origin, dtype=torch.float64, device=p.device) + h * v.to(torch.float64)).contiguous()
    _, t["density"] = timed(lambda: ops.poisson_sample(W, origin, h, verts))
    return t, dict(dims=list(dims), h=h, info=info, vertices=int(v.shape[0]), faces=int(f.shape[0]), b=b, verts=verts)


def torch_cg(b, h, iterations):
    """the same three steps per iteration as torch fp64 operations; the scalars stay on the device"""
    import torch.nn.functional as F

    def A(p):
        f = F.pad(p, (1, 1, 1, 1, 1, 1))
        s = ((f[:-2, 1:-1, 1:-1] + f[2:, 1:-1, 1:-1]) + (f[1:-1, :-2, 1:-1] + f[1:-1, 2:, 1:-1])) + (f[1:-1, 1:-1, :-2] + f[1:-1, 1:-1, 2:])
        return (6.0 * p - s) / (h * h)

    x = torch.zeros_like(b)
    r = -b
    p = r.clone()
    rr = (r * r).sum()
    for _ in range(iterations):
        q = A(p)
        alpha = rr / (p * q).sum()
        x += alpha * p
        r -= alpha * q
        rr_new = (r * r).sum()
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x, torch.sqrt(rr)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(np.min(vals)), max=float(np.max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm, as bench_pcd_filter")
    ap.add_argument("--noise", type=float, default=1e-3, help="radial noise as a share of the radius")
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--pad", type=int, default=4)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host_cg_at", type=int, default=128, help="resolution of the scipy comparison (0: skip it)")
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_poisson: no GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    d = rng.normal(size=(a.points, 3))
    radius = a.radius * VOXEL
    nrm = d / np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.ascontiguousarray(nrm * radius * (1.0 + a.noise * rng.standard_normal(a.points))[:, None])
    p, n = torch.from_numpy(pts).cuda(), torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, warmup_runs=1, tol=a.tol, pad=a.pad,
               cloud=f"{a.points} points on a sphere of {radius} mm, radial noise {a.noise * radius} mm, exact outward normals",
               bytes_per_node_and_iteration=BYTES_PER_NODE, hbm_bytes_per_s_measured_streaming=HBM_MEASURED,
               note="synthetic cloud: no real scan and no trained checkpoint has been reconstructed")
    for resolution in a.resolutions:
        stages(p, n, resolution, a.pad, a.tol)                                    # warm-up: code objects, allocator
        runs = [stages(p, n, resolution, a.pad, a.tol) for _ in range(a.runs)]
        facts = runs[-1][1]
        nodes = int(np.prod(facts["dims"]))
        it = facts["info"]["iterations"]
        item = dict(dims=facts["dims"], nodes=nodes, h_mm=facts["h"], vertices=facts["vertices"], faces=facts["faces"],
                    iterations=it, residual=facts["info"]["residual"], converged=facts["info"]["converged"],
                    stage_ms={k: spread([r[0][k] for r in runs]) for k in runs[0][0]},
                    total_ms=spread([sum(r[0].values()) for r in runs]))
        per_it = [r[0]["solve"] / max(it, 1) for r in runs]
        item["cg_ms_per_iteration"] = spread(per_it)
        item["cg_bytes_per_s"] = BYTES_PER_NODE * nodes / (np.median(per_it) * 1e-3)
        item["cg_share_of_measured_hbm"] = item["cg_bytes_per_s"] / HBM_MEASURED
        err = np.abs(np.linalg.norm(facts["verts"].cpu().numpy(), axis=1) - radius) / facts["h"]
        item["worst_vertex_distance_to_the_sphere_in_h"] = float(err.max())
        b, h = facts["b"], facts["h"]
        torch_cg(b, h, 4)                                                         # warm-up
        tt = [timed(lambda: torch_cg(b, h, it))[1] for _ in range(max(a.runs // 2, 2))]
        item["torch_fp64_cg_same_iterations_ms"] = spread(tt)
        item["torch_fp64_cg_ms_per_iteration"] = float(np.median(tt) / max(it, 1))
        if resolution == a.host_cg_at:
            from scipy.sparse.linalg import cg

            A = R.matrix(facts["dims"], h)
            rhs = -b.cpu().numpy().reshape(-1)
            count = [0]
            t0 = time.perf_counter()
            x, flag = cg(A, rhs, rtol=a.tol, maxiter=8 * max(facts["dims"]), callback=lambda _: count.__setitem__(0, count[0] + 1))
            item["host_scipy_cg"] = dict(ms=(time.perf_counter() - t0) * 1e3, iterations=count[0], flag=int(flag), runs=1)
        res[f"resolution_{resolution}"] = item
        del runs, facts, b
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
