"""Benchmark of mesh simplification (uforecon_amd/simplify_mesh.py, csrc/mesh_simplify.hip): the marching-cubes sphere of about
2 M vertices of the other mesh benchmarks, simplified to 0.25, 0.1 and 0.01 of its vertices.
  * per ratio: the bisection for the cell alone, the stages of ``ops.mesh_simplify`` at that cell by wall clock (each ended by
    a device synchronise), the call end to end, and HIP events around every launch (ufr_profile_*) in a run of its own;
  * the same rule as torch float64 operations on the same device (``unique``, ``index_add_``, a batched solve): it need not
    match bit for bit -- its sums are unordered -- and is there for scale; the vertex and face counts are compared;
  * quality, both placements: on the sphere the mean and the largest | |v| - R |, on a tessellated unit cube the largest
    distance of an output vertex to the cube's surface.
Nothing earlier exists to compare with, so no threshold is set.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_clean_mesh import VOXEL, sphere_mesh  # noqa: E402
from uforecon_amd import ops  # noqa: E402

RATIOS = (0.25, 0.1, 0.01)


def cube_mesh(n=65):
    """the unit cube's surface, n x n vertices per side (the sides do not share vertices: clustering merges them anyway)"""
    g = np.linspace(0.0, 1.0, n)
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij"))
    q = np.stack([i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1], 1)
    verts, faces = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            p = np.empty((n * n, 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = side, a, b
            qq = q if side else q[:, ::-1]
            faces.append(np.concatenate([qq[:, [0, 1, 2]], qq[:, [0, 2, 3]]]) + len(verts) * n * n)
            verts.append(p)
    return np.concatenate(verts), np.ascontiguousarray(np.concatenate(faces).astype(np.int32))


def cube_distance(p):
    out = np.linalg.norm(np.maximum(np.maximum(p - 1.0, -p), 0.0), axis=1)
    inside = np.minimum(p, 1.0 - p).min(1)
    return np.where(out > 0, out, np.maximum(inside, 0.0))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def staged(tv, tf, cell, placement="quadric"):
    """ops.mesh_simplify's calls, one by one, with the wall clock of each"""
    ms = {}
    mn, mx = tv.min(0).values, tv.max(0).values
    (origin, keys, order), ms["vertex_keys_sort_ms"] = timed(lambda: ops._simplify_sorted_keys(tv, mn, mx, cell, "bench"))
    (cluster, ckey), ms["clusters_ms"] = timed(lambda: ops.simplify_clusters(keys, order))
    (mean, _, _, count), ms["voxel_mean_ms"] = timed(lambda: ops.voxel_downsample(tv, cell))      # keys and sort once more
    fkeys, ms["face_keys_sort_ms"] = timed(lambda: torch.sort(ops.simplify_face_keys(tf, cluster), stable=True).values)
    (Q, nf), ms["quadrics_ms"] = timed(lambda: ops.simplify_quadrics(tv, tf, ckey, origin, cell, fkeys))
    (pos, placed), ms["place_ms"] = timed(lambda: ops.simplify_place(Q, nf, mean, ckey, origin, cell, placement))
    (tri, ka, kbc), ms["face_triples_ms"] = timed(lambda: ops.simplify_face_triples(tf, cluster))
    keep, ms["face_sorts_heads_ms"] = timed(lambda: ops.simplify_face_heads(ka, kbc))
    (of, fmap, ref), ms["compact_faces_ms"] = timed(lambda: ops.simplify_compact_faces(tri, keep, len(ckey)))
    _, ms["compact_vertices_ms"] = timed(lambda: ops.simplify_compact_vertices(ref, pos, None, placed, count, cluster, of))
    return ms


def torch_same_rule(tv, tf, cell):
    """vertex clustering with the regularised quadric as torch float64 operations; returns (verts, faces)"""
    origin = tv.min(0).values - cell / 2
    ijk = torch.floor((tv - origin) / cell).long()
    dims = ijk.max(0).values + 1
    lin = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
    ukey, cluster = torch.unique(lin, return_inverse=True)
    C = len(ukey)
    cnt = torch.zeros(C, dtype=torch.float64, device=tv.device).index_add_(0, cluster, torch.ones_like(tv[:, 0]))
    mean = torch.zeros((C, 3), dtype=torch.float64, device=tv.device).index_add_(0, cluster, tv) / cnt[:, None]
    cijk = torch.stack([ukey // (dims[1] * dims[2]), (ukey // dims[2]) % dims[1], ukey % dims[2]], 1).double()
    centre = origin + (cijk + 0.5) * cell
    c = cluster[tf.long()]
    pa, pb, pc = tv[tf[:, 0].long()], tv[tf[:, 1].long()], tv[tf[:, 2].long()]
    n = torch.linalg.cross(pb - pa, pc - pa)
    Q = torch.zeros((C, 10), dtype=torch.float64, device=tv.device)
    for e, sel in ((0, None), (1, c[:, 1] != c[:, 0]), (2, (c[:, 2] != c[:, 0]) & (c[:, 2] != c[:, 1]))):
        ce, ne, ae = (c[:, e], n, pa) if sel is None else (c[sel, e], n[sel], pa[sel])
        d = -(ne * (ae - centre[ce])).sum(1)
        terms = torch.stack([ne[:, 0] * ne[:, 0], ne[:, 0] * ne[:, 1], ne[:, 0] * ne[:, 2], ne[:, 1] * ne[:, 1], ne[:, 1] * ne[:, 2],
                             ne[:, 2] * ne[:, 2], ne[:, 0] * d, ne[:, 1] * d, ne[:, 2] * d, d * d], 1)
        Q.index_add_(0, ce, terms)
    xb = mean - centre
    w = 2.0 ** -10 * (Q[:, 0] + Q[:, 3] + Q[:, 5])
    A = torch.stack([Q[:, 0] + w, Q[:, 1], Q[:, 2], Q[:, 1], Q[:, 3] + w, Q[:, 4], Q[:, 2], Q[:, 4], Q[:, 5] + w], 1).reshape(C, 3, 3)
    b = Q[:, 6:9] - w[:, None] * xb
    ok = w > 0
    safe = torch.where(ok[:, None, None], A, torch.eye(3, dtype=torch.float64, device=tv.device)[None])
    x = torch.linalg.solve(safe, -b[:, :, None])[:, :, 0]

    def err(y):
        return (y * (A @ y[:, :, None])[:, :, 0]).sum(1) + 2.0 * (b * y).sum(1)

    take = ok & torch.isfinite(x).all(1) & (x.abs() <= 0.5 * cell).all(1) & (err(x) <= err(xb))
    pos = torch.where(take[:, None], centre + x, mean)
    good = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    c = c[good]
    first = c.argmin(1)
    rot = torch.stack([c.gather(1, ((first + e) % 3)[:, None])[:, 0] for e in range(3)], 1)
    rot = torch.unique(rot, dim=0)
    used, faces = torch.unique(rot, return_inverse=True)
    return pos[used], faces.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=320, help="sphere radius in voxels of 1.5 mm (320: a mesh of about 2 M vertices)")
    ap.add_argument("--cube", type=int, default=65, help="vertices per side of the cube")
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    verts, faces = sphere_mesh(a.radius)
    R_mm = a.radius * VOXEL
    dev = torch.device("cuda")
    tv, tf = torch.from_numpy(verts).to(dev), torch.from_numpy(faces.astype(np.int32)).to(dev)
    V = len(verts)
    ops.mesh_simplify(tv, tf[:4096].contiguous(), cell=10.0)                                       # warm: library, allocator
    res = dict(mesh=f"{V} vertices, {len(faces)} faces, a sphere of {R_mm} mm", runs=1, ratios={})
    for ratio in RATIOS:
        N = int(math.ceil(ratio * V))
        r = {}
        cell, r["bisection_ms"] = timed(lambda: ops.simplify_target_cell(tv, N))
        r["cell_mm"], r["target_vertices"] = cell, N
        ops.mesh_simplify(tv, tf, cell=cell)                                                    # warm at this size
        out, r["simplify_at_cell_ms"] = timed(lambda: ops.mesh_simplify(tv, tf, cell=cell))
        _, r["end_to_end_target_ms"] = timed(lambda: ops.mesh_simplify(tv, tf, target_vertices=N))
        r["stages"] = staged(tv, tf, cell)
        ops.profile_enable(True)
        ops.mesh_simplify(tv, tf, cell=cell)
        torch.cuda.synchronize()
        prof = ops.profile_read()
        ops.profile_enable(False)
        r["kernels_ms"] = {k: dict(ms=v["ms"], launches=v["launches"]) for k, v in prof.items()}
        r.update(vertices_out=int(len(out["verts"])), faces_out=int(len(out["faces"])), clusters=out["clusters"],
                 collapsed_faces=out["collapsed_faces"], duplicate_faces=out["duplicate_faces"],
                 quadric_share=float(out["placed"].double().mean()))
        torch_same_rule(tv, tf, cell)                                                           # warm
        (tverts, tfaces), t_ms = timed(lambda: torch_same_rule(tv, tf, cell))
        r["torch_same_rule"] = dict(ms=t_ms, times_the_call=t_ms / r["simplify_at_cell_ms"], vertices=int(len(tverts)),
                                    faces=int(len(tfaces)), vertices_equal=int(len(tverts)) == r["vertices_out"],
                                    faces_equal=int(len(tfaces)) == r["faces_out"])
        q = {}
        for placement in ("quadric", "mean"):
            o = out if placement == "quadric" else ops.mesh_simplify(tv, tf, cell=cell, placement=placement)
            e = (o["verts"].norm(dim=1) - R_mm).abs()
            q[placement] = dict(mean_radial_error_mm=float(e.mean()), max_radial_error_mm=float(e.max()))
        r["sphere_quality"] = q
        res["ratios"][str(ratio)] = r
    cv, cf = cube_mesh(a.cube)
    tcv, tcf = torch.from_numpy(cv).to(dev), torch.from_numpy(cf).to(dev)
    cube = {}
    for cell in (0.3, 0.1):
        for placement in ("quadric", "mean"):
            o = ops.mesh_simplify(tcv, tcf, cell=cell, placement=placement)
            d = cube_distance(o["verts"].cpu().numpy())
            cube[f"cell_{cell}_{placement}"] = dict(vertices_out=int(len(d)), max_distance_to_surface=float(d.max()),
                                                    mean_distance_to_surface=float(d.mean()),
                                                    quadric_share=float(o["placed"].double().mean()))
    res["cube"] = dict(mesh=f"{len(cv)} vertices, {len(cf)} faces, the unit cube", **cube)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
