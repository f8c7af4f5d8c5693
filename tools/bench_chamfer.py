"""Benchmark of the DTU chamfer evaluation (uforecon_amd/dtu_eval.py, csrc/chamfer.hip) on a synthetic scan of realistic
size: the marching-cubes mesh of tools/bench_tsdf.py's wall scene, scaled so that sampling at density 0.2 gives about
--points points (default 10 M), against a ground-truth cloud of about --gt-points (default 3 M: the mesh sampled more
coarsely, with noise and a hole).

Reports per-stage kernel time from ufr_profile_* (mesh sampling, cell keys, the thinning rounds and their number, the two
nearest-neighbour passes), points per second per stage, and the end-to-end time of dtu_eval.chamfer() (which includes
torch's sorts and gathers and the host synchronisations).

For comparison the CPU route on the same host in the same run, at --cpu-points (default 200 k: the full size takes many
minutes on a CPU), next to chamfer() at that same size: where sklearn is importable the reference's own calls (kd-tree
radius query + the Python loop + two kneighbors), otherwise the numpy restatement (tests/chamfer_ref.py)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_ref as R  # noqa: E402
from bench_tsdf import scene  # noqa: E402
from uforecon_amd import dtu_eval, ops, tsdf  # noqa: E402

DENSITY, MAX_DIST = 0.2, 20.0
STAGES = ("mesh_sample_count", "mesh_sample_scan", "mesh_sample_emit", "points_cell_keys", "points_thin_round", "points_nn_dist")


def wall_mesh(n):
    K, P, depth, bnds, vs = scene(n)
    vol = tsdf.TSDFVolume(bnds.copy(), voxel_size=vs, margin=3)
    vol.integrate(None, torch.from_numpy(depth).cuda(), K, P)
    verts, faces, _, _ = vol.get_mesh()
    return verts.astype(np.float64), faces


def make_scan(verts, faces, points, gt_points, seed=0):
    """the mesh scaled to ``points`` samples at DENSITY, a ground truth of about ``gt_points``, mask / box / plane that keep
    almost everything (their cost is negligible; the golden fixtures test them)"""
    tv = verts[faces]
    area = 0.5 * np.linalg.norm(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]), axis=1).sum()
    v = verts * np.sqrt(points * DENSITY ** 2 / area)               # samples ~ area / density^2
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(faces).cuda()
    gt = ops.sample_mesh(vt, ft, DENSITY * np.sqrt(points / gt_points))
    g = torch.Generator(device="cuda").manual_seed(seed)
    gt = gt + torch.randn(gt.shape, generator=g, device="cuda", dtype=torch.float64) * 0.1
    lo, hi = v.min(0), v.max(0)
    hole = ((gt[:, :2] - torch.from_numpy((lo + 0.3 * (hi - lo))[:2]).cuda()).norm(dim=1) < 0.1 * float((hi - lo).max()))
    gt = gt[~hole].to(torch.float32).cpu().numpy()
    res = float((hi - lo).max()) / 64
    bb = np.stack([lo - 2 * res, hi + 2 * res])
    shape = tuple(int(s) for s in np.ceil((bb[1] - bb[0]) / res) + 1)
    obs = np.ones(shape, np.uint8)
    obs[:4] = 0
    return dict(verts=v, faces=faces, gt=gt, obs=obs, bb=bb, res=res, plane=np.array([0.0, 0.0, 1.0, 1e6]))


def gpu_run(s, reps):
    kw = dict(density=DENSITY, patch=60, max_dist=MAX_DIST, seed=0)
    out = dtu_eval.chamfer((s["verts"], s["faces"]), s["gt"], s["obs"], s["bb"], s["res"], s["plane"], **kw)     # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        dtu_eval.chamfer((s["verts"], s["faces"]), s["gt"], s["obs"], s["bb"], s["res"], s["plane"], **kw)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) / reps
    ops.profile_enable(True)
    ops.profile_read()
    dtu_eval.chamfer((s["verts"], s["faces"]), s["gt"], s["obs"], s["bb"], s["res"], s["plane"], **kw)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    return out, wall, {k: prof.get(k, dict(ms=0.0, launches=0)) for k in STAGES}


def cpu_run(s):
    """the reference's route on the CPU: (seconds per stage, d2s, s2d, which)"""
    t = {}
    t0 = time.perf_counter()
    pcd = R.sample_mesh(s["verts"], s["faces"], DENSITY)
    pcd = pcd[np.random.default_rng(0).permutation(len(pcd))]
    t["sample"] = time.perf_counter() - t0
    stl = s["gt"].astype(np.float64)
    try:
        import sklearn.neighbors as skln
    except ImportError:
        skln = None
    t0 = time.perf_counter()
    if skln is not None:
        nn_engine = skln.NearestNeighbors(n_neighbors=1, radius=DENSITY, algorithm="kd_tree",
                                           n_jobs=int(os.environ.get("OMP_NUM_THREADS", 0)) or -1)   # the reference: -1
        nn_engine.fit(pcd)
        rnn_idxs = nn_engine.radius_neighbors(pcd, radius=DENSITY, return_distance=False)
        mask = np.ones(pcd.shape[0], dtype=np.bool_)
        for curr, idxs in enumerate(rnn_idxs):
            if mask[curr]:
                mask[idxs] = 0
                mask[curr] = 1
    else:
        mask = R.thin_grid(pcd, DENSITY)
    t["thin"] = time.perf_counter() - t0
    down = pcd[mask]
    inbound, grid_inbound, in_obs = R.observation_filter(down, s["obs"], s["bb"], s["res"], 60.0)
    data_in = down[inbound]
    data_in_obs = data_in[grid_inbound][in_obs]
    above = stl[(s["plane"].reshape(1, 4) * np.concatenate([stl, np.ones_like(stl[:, :1])], -1)).sum(-1) > 0]
    t0 = time.perf_counter()
    if skln is not None:
        nn_engine.fit(stl)
        d2s = nn_engine.kneighbors(data_in_obs, n_neighbors=1, return_distance=True)[0]
        nn_engine.fit(data_in)
        s2d = nn_engine.kneighbors(above, n_neighbors=1, return_distance=True)[0]
    else:
        d2s, s2d = R.nn_grid(data_in_obs, stl, MAX_DIST), R.nn_grid(above, data_in, MAX_DIST)
    t["nn"] = time.perf_counter() - t0
    return t, float(d2s[d2s < MAX_DIST].mean()), float(s2d[s2d < MAX_DIST].mean()), "sklearn kd_tree" if skln is not None else "numpy restatement"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="TSDF volume side of the wall scene")
    ap.add_argument("--points", type=float, default=10e6)
    ap.add_argument("--gt-points", type=float, default=3e6)
    ap.add_argument("--cpu-points", type=float, default=2e5, help="size of the CPU comparison (0: skip it)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", help="also write the result as JSON to this path")
    a = ap.parse_args()
    verts, faces = wall_mesh(a.n)
    s = make_scan(verts, faces, a.points, a.gt_points)
    out, wall, prof = gpu_run(s, a.reps)
    c = out["counts"]
    items = dict(mesh_sample_count=len(faces), mesh_sample_scan=len(faces), mesh_sample_emit=c["sampled"],
                 points_cell_keys=c["sampled"] + c["in_obs"] + c["gt"] + c["gt_above"] + c["in_box"],
                 points_thin_round=c["sampled"], points_nn_dist=c["in_obs"] + c["gt_above"])
    res = dict(device=torch.cuda.get_device_name(0), faces=int(len(faces)), counts=c, thin_rounds=out["thin_rounds"],
               d2s=out["d2s"], s2d=out["s2d"], chamfer_s=wall,
               kernel_ms={k: round(v["ms"], 3) for k, v in prof.items()}, launches={k: v["launches"] for k, v in prof.items()},
               kernels_ms=sum(v["ms"] for v in prof.values()),
               items_per_s={k: (items[k] / (prof[k]["ms"] * 1e-3) if prof[k]["ms"] else None) for k in STAGES})
    print(f"{len(faces)} triangles -> {c['sampled']} points, {c['thinned']} after {out['thin_rounds']} thinning rounds, "
          f"{c['in_obs']} x {c['gt']} (d2s), {c['gt_above']} x {c['in_box']} (s2d): d2s {out['d2s']:.6f} s2d {out['s2d']:.6f}")
    for k in STAGES:
        ips = res["items_per_s"][k]
        print(f"  {k:18s} {prof[k]['ms']:9.3f} ms in {prof[k]['launches']:3d} launches" + (f"   {ips / 1e6:9.1f} M items/s" if ips else ""))
    print(f"  kernels            {res['kernels_ms']:9.3f} ms;  dtu_eval.chamfer() end to end {wall * 1e3:.1f} ms")
    if a.cpu_points > 0:
        sc = make_scan(verts, faces, a.cpu_points, a.cpu_points * a.gt_points / a.points)
        gout, gwall, _ = gpu_run(sc, a.reps)
        t, d2s, s2d, which = cpu_run(sc)
        res["cpu_comparison"] = dict(route=which, points=gout["counts"]["sampled"], gt=gout["counts"]["gt"], cpu_s=t, cpu_total_s=sum(t.values()),
                                     gpu_chamfer_s=gwall, d2s=(d2s, gout["d2s"]), s2d=(s2d, gout["s2d"]))
        print(f"CPU route ({which}) at {gout['counts']['sampled']} points x {gout['counts']['gt']} ground truth: sample {t['sample']:.2f} s, "
              f"thin {t['thin']:.2f} s, nn {t['nn']:.2f} s = {sum(t.values()):.2f} s; chamfer() at the same size {gwall * 1e3:.1f} ms "
              f"({sum(t.values()) / gwall:.0f} x); d2s {d2s:.9f} vs {gout['d2s']:.9f}, s2d {s2d:.9f} vs {gout['s2d']:.9f}")
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
