"""DTU chamfer evaluation on the GPU: the reference's evaluation/dtu_eval.py (both --mode mesh and --mode pcd) with its
point sampling, thinning and nearest-neighbour passes as HIP kernels (csrc/chamfer.hip through ``ops.sample_mesh``,
``ops.thin_points``, ``ops.nn_distance``), in float64 as the reference computes.

    python -m uforecon_amd.dtu_eval --outdir OUT --dataset_dir MVS_Data [--mode mesh|pcd] [--mesh_dir OUT/mesh]

takes the reference's flags and paths and appends the reference's lines to ``<outdir>/eval_final.log``.  The one
difference: the reference shuffles the cloud with an unseeded generator, here the permutation is
``numpy.random.default_rng(seed).permutation(N)`` (``--seed``, default 0), so a run can be repeated.  ``--write_vis`` adds what
the reference only describes in a commented-out block: the error-coloured clouds ``<vis_out_dir>/vis_<scan:03>_d2s.ply`` and
``..._s2d.ply`` (``error_clouds``), which ``python -m uforecon_amd.render_trajectory --ply`` renders.

Inputs of any float dtype are converted to float64 once on entry, as the reference sees the text of a PLY file as
float64; ``chamfer()`` on an in-memory fp32 mesh and the command line on its ``%f``-formatted PLY file may therefore differ
in the seventh digit.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys

import numpy as np

DTU_SCANS = [24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122]

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path: str, with_colors: bool = False, with_normals: bool = False):
    """(vertices (V,3) float64, faces (F,3) int32 or None) of an ASCII or binary_little_endian PLY file: vertex x / y / z as
    float or double (other vertex properties are skipped), faces as ``list uchar int|uint`` triangles.  Elements after the
    faces are ignored.  ``with_colors``: a third item, the vertex properties red / green / blue (uchar) as (V,3) uint8, or None
    when the file has none.  ``with_normals``: one more item, the vertex properties nx / ny / nz (float or double) as (V,3)
    float64, or None when the file has none."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body_at = raw.index(b"\n", end) + 1
    header = raw[:end].decode("ascii", "replace").split("\n")
    fmt = None
    elements = []                                   # [name, count, [(kind, type, name) ...]]
    for line in header:
        t = line.split()
        if not t:
            continue
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            elements.append([t[1], int(t[2]), []])
        elif t[0] == "property":
            if t[1] == "list":
                elements[-1][2].append(("list", (t[2], t[3]), t[4]))
            else:
                elements[-1][2].append(("scalar", t[1], t[2]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii and binary_little_endian are)")
    verts, faces, colors, normals = None, None, None, None
    tokens = raw[body_at:].split() if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else body_at
    for name, count, props in elements:
        if name == "vertex":
            if any(k != "scalar" for k, _, _ in props):
                raise ValueError(f"{path}: list property in the vertex element")
            names = [n for _, _, n in props]
            if not all(a in names for a in "xyz"):
                raise ValueError(f"{path}: vertex element without x, y, z")
            cols = [names.index(a) for a in "xyz"]
            if any(props[c][1] not in ("float", "float32", "double", "float64") for c in cols):
                raise ValueError(f"{path}: x, y, z must be float or double")
            rgb = ("red", "green", "blue")
            has_rgb = all(a in names and _PLY_TYPES.get(props[names.index(a)][1]) == "u1" for a in rgb)
            nxyz = ("nx", "ny", "nz")
            has_n = with_normals and all(a in names and _PLY_TYPES.get(props[names.index(a)][1]) in ("f4", "f8") for a in nxyz)
            if fmt == "ascii":
                rows = np.array(tokens[pos:pos + count * len(props)], dtype="S").astype(np.float64).reshape(count, len(props))
                verts = rows[:, cols] if count else np.zeros((0, 3))
                if has_rgb:
                    colors = rows[:, [names.index(a) for a in rgb]].astype(np.uint8) if count else np.zeros((0, 3), np.uint8)
                if has_n:
                    normals = rows[:, [names.index(a) for a in nxyz]] if count else np.zeros((0, 3))
                pos += count * len(props)
            else:
                dt = np.dtype([(n, "<" + _PLY_TYPES[t]) for _, t, n in props])
                rec = np.frombuffer(raw, dt, count, pos)
                verts = np.stack([rec[a].astype(np.float64) for a in "xyz"], 1) if count else np.zeros((0, 3))
                if has_rgb:
                    colors = np.stack([rec[a] for a in rgb], 1) if count else np.zeros((0, 3), np.uint8)
                if has_n:
                    normals = np.stack([rec[a].astype(np.float64) for a in nxyz], 1) if count else np.zeros((0, 3))
                pos += count * dt.itemsize
        elif name == "face":
            if len(props) != 1 or props[0][0] != "list" or _PLY_TYPES.get(props[0][1][1]) not in ("i4", "u4"):
                raise ValueError(f"{path}: faces must be one `list uchar int` (or uint) property")
            if fmt == "ascii":
                rows = np.array(tokens[pos:pos + 4 * count], dtype="S").astype(np.int64).reshape(count, 4) if count else np.zeros((0, 4), np.int64)
                if (rows[:, 0] != 3).any():
                    raise ValueError(f"{path}: only triangle faces are supported")
                faces = rows[:, 1:].astype(np.int32)
                pos += 4 * count
            else:
                dt = np.dtype([("n", "<" + _PLY_TYPES[props[0][1][0]]), ("v", "<" + _PLY_TYPES[props[0][1][1]], (3,))])
                rec = np.frombuffer(raw, dt, count, pos)
                if (rec["n"] != 3).any():
                    raise ValueError(f"{path}: only triangle faces are supported")
                faces = rec["v"].astype(np.int32)
                pos += count * dt.itemsize
            break
        else:
            if verts is None:
                raise ValueError(f"{path}: element {name!r} before the vertices is not supported")
            break
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return (verts, faces) + ((colors,) if with_colors else ()) + ((normals,) if with_normals else ())


def _load_arrays(path: str, names):
    """the named arrays of a .mat file (scipy, imported on demand) or an .npz file"""
    if path.endswith(".npz"):
        z = np.load(path)
        return [np.asarray(z[n]) for n in names]
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise RuntimeError(f"{path}: reading .mat files needs scipy (pip package `scipy`); the same arrays are also "
                           f"accepted as an .npz file with the keys {list(names)}") from e
    m = loadmat(path)
    return [np.asarray(m[n]) for n in names]


def _pick(base: str) -> str:
    """base + '.mat', or base + '.npz' when only that exists"""
    return base + ".npz" if not os.path.exists(base + ".mat") and os.path.exists(base + ".npz") else base + ".mat"


def chamfer(data, gt_points, obs_mask, bb, res, plane, *, density: float = 0.2, patch: float = 60, max_dist: float = 20,
            seed: int = 0, details: bool = False) -> dict:
    """dtu_eval.py's loop body for one scan.  ``data``: ``(verts, faces)`` (--mode mesh) or a point array (--mode pcd);
    ``gt_points`` the ground-truth cloud; ``obs_mask`` / ``bb`` (2,3) / ``res`` the arrays of ObsMask*_10.mat; ``plane`` the
    four coefficients of Plane*.mat.  numpy arrays or tensors, any float dtype.  Returns d2s, s2d, overall (python floats;
    nan when a set is empty), the point counts at every stage and the number of thinning rounds; with ``details`` also the
    distance tensors and masks (CUDA)."""
    import torch

    from . import ops
    from ._lib import UfrError

    if not torch.cuda.is_available():
        raise UfrError("dtu_eval.chamfer: needs a GPU (the sampling, thinning and nearest-neighbour passes are HIP kernels)")
    dev = torch.device("cuda")

    def f64(a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()

    density, patch, max_dist = float(density), float(patch), float(max_dist)
    if isinstance(data, (tuple, list)):
        verts, faces = data
        faces = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
        data_pcd = ops.sample_mesh(f64(verts), faces.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous(), density)
    else:
        data_pcd = f64(data)
    n_sampled = int(data_pcd.shape[0])
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(n_sampled)).to(dev)
    data_pcd = data_pcd[perm].contiguous()
    keep, rounds = ops.thin_points(data_pcd, density, return_rounds=True)
    data_down = data_pcd[keep]

    # the box and grid tests with the reference's dtypes: BB is cast to float32 and offset in float32 [121-124]
    BB = np.asarray(bb.cpu() if isinstance(bb, torch.Tensor) else bb).reshape(2, 3).astype(np.float32)
    lo = torch.from_numpy((BB[:1] - np.float32(patch)).astype(np.float64)).to(dev)
    hi = torch.from_numpy((BB[1:] + np.float32(patch * 2)).astype(np.float64)).to(dev)
    inbound = ((data_down >= lo) & (data_down < hi)).all(-1)
    data_in = data_down[inbound].contiguous()
    mask = obs_mask if isinstance(obs_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(obs_mask))
    mask = mask.to(dev) != 0
    res = float(np.asarray(res.cpu() if isinstance(res, torch.Tensor) else res).reshape(-1)[0])
    grid = torch.round((data_in - torch.from_numpy(BB[:1].astype(np.float64)).to(dev)) / res).to(torch.int64)     # half to even
    dims = torch.tensor(list(mask.shape), device=dev)
    grid_inbound = ((grid >= 0) & (grid < dims)).all(-1)
    g = grid[grid_inbound]
    in_obs = mask[g[:, 0], g[:, 1], g[:, 2]]
    data_in_obs = data_in[grid_inbound][in_obs].contiguous()

    stl = f64(gt_points)
    P = [float(v) for v in np.asarray(plane.cpu() if isinstance(plane, torch.Tensor) else plane, np.float64).reshape(-1)]
    above = (((stl[:, 0] * P[0] + stl[:, 1] * P[1]) + stl[:, 2] * P[2]) + P[3]) > 0
    stl_above = stl[above].contiguous()

    def mean_nn(query, ref):
        if query.shape[0] == 0 or ref.shape[0] == 0:
            return torch.full((query.shape[0],), float("inf"), dtype=torch.float64, device=dev), float("nan")
        d, sums = ops.nn_distance(query, ref, max_dist, return_sums=True)
        s, c = sums.tolist()
        return d, (s / c if c > 0 else float("nan"))

    dist_d2s, d2s = mean_nn(data_in_obs, stl)
    dist_s2d, s2d = mean_nn(stl_above, data_in)
    out = dict(d2s=d2s, s2d=s2d, overall=(d2s + s2d) / 2, thin_rounds=rounds,
               counts=dict(sampled=n_sampled, thinned=int(data_down.shape[0]), in_box=int(data_in.shape[0]),
                           in_grid=int(g.shape[0]), in_obs=int(data_in_obs.shape[0]), gt=int(stl.shape[0]),
                           gt_above=int(stl_above.shape[0])))
    if details:
        out.update(data_pcd=data_pcd, thin_mask=keep, inbound=inbound, grid_inbound=grid_inbound, in_obs=in_obs, above=above,
                   dist_d2s=dist_d2s, dist_s2d=dist_s2d)
    return out


def error_clouds(result: dict, gt_points, max_dist: float = 20, vis_dist: float = 10):
    """The error-coloured clouds of one scan, ``((points, colors), (points, colors))`` for d2s and s2d, from the result of
    ``chamfer(..., details=True)``: float64 (n,3) points and uint8 (n,3) colours, tensors on the device the result's tensors
    live on (torch ops only; CPU tensors work).  The rule is the one the reference's evaluation/dtu_eval.py describes in a
    commented-out block (:159-173), in this module's names:

    * d2s: every point of the thinned cloud ``data_pcd[thin_mask]``, blue; the points that passed the box, the grid and ObsMask
      -- the ones ``dist_d2s`` belongs to, in its order -- get ``a = min(dist, vis_dist) / vis_dist`` and the colour
      ``(1, 1 - a, 1 - a)``, white to red; those with ``dist >= max_dist`` (infinite included) are green;
    * s2d: every ground-truth point, blue; the points above the plane are coloured the same way by ``dist_s2d``.

    Bytes are ``rint(255 c)`` in float64, round half to even."""
    import torch

    max_dist, vis_dist = float(max_dist), float(vis_dist)
    if not vis_dist > 0:
        raise ValueError(f"error_clouds: vis_dist {vis_dist} (must be positive)")
    data_down = result["data_pcd"][result["thin_mask"]]
    dev = data_down.device
    gt = gt_points if isinstance(gt_points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(gt_points))
    gt = gt.to(device=dev, dtype=torch.float64).reshape(-1, 3)

    def paint(n, where, dist):
        col = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        col[:, 2] = 1.0                                                       # blue
        dist = dist.to(torch.float64).reshape(-1)
        a = torch.clamp(dist, max=vis_dist) / vis_dist
        ramp = torch.stack([torch.ones_like(a), 1.0 - a, 1.0 - a], 1)
        ramp[dist >= max_dist] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=dev)   # green
        col[where] = ramp
        return torch.round(255.0 * col).to(torch.uint8)                       # half to even

    idx = torch.nonzero(result["inbound"]).reshape(-1)[result["grid_inbound"]][result["in_obs"]]
    above = torch.nonzero(result["above"]).reshape(-1)
    return ((data_down, paint(data_down.shape[0], idx, result["dist_d2s"])),
            (gt, paint(gt.shape[0], above, result["dist_s2d"])))


def write_ply_points(filename: str, points, colors) -> None:
    """binary little-endian PLY of a coloured cloud: double x / y / z, uchar red / green / blue (``read_ply(...,
    with_colors=True)`` reads it back bit for bit)"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    colors = np.asarray(colors).reshape(-1, 3)
    if colors.dtype != np.uint8 or len(colors) != len(points):
        raise ValueError(f"write_ply_points: colors {colors.shape} {colors.dtype}: expected ({len(points)}, 3) uint8")
    rec = np.empty(len(points), dtype=[("p", "<f8", (3,)), ("c", "u1", (3,))])
    rec["p"] = points
    rec["c"] = colors
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(rec))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def evaluate_scan(data_path: str, mode: str, gt_path: str, obs_path: str, plane_path: str, vis_prefix=None, vis_dist: float = 10,
                  **kw) -> dict:
    """``chamfer`` on files: a mesh or point-cloud PLY, the ground-truth PLY, ObsMask*_10.mat and Plane*.mat (or .npz files
    with the same keys).  With ``vis_prefix`` the error clouds (``error_clouds``) go to ``<vis_prefix>_d2s.ply`` and
    ``<vis_prefix>_s2d.ply``; the scores are the same either way."""
    verts, faces = read_ply(data_path)
    if mode == "mesh":
        if faces is None:
            raise ValueError(f"{data_path}: --mode mesh needs a PLY file with faces")
        data = (verts, faces)
    else:
        data = verts
    gt, _ = read_ply(gt_path)
    obs_mask, bb, res = _load_arrays(obs_path, ["ObsMask", "BB", "Res"])
    (plane,) = _load_arrays(plane_path, ["P"])
    if vis_prefix is None:
        return chamfer(data, gt, obs_mask, bb, res, plane, **kw)
    r = chamfer(data, gt, obs_mask, bb, res, plane, details=True, **kw)
    clouds = error_clouds(r, gt, max_dist=kw.get("max_dist", 20), vis_dist=vis_dist)
    for name, (pts, col) in zip(("d2s", "s2d"), clouds):
        write_ply_points(f"{vis_prefix}_{name}.ply", pts.cpu().numpy(), col.cpu().numpy())
    return r


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="DTU chamfer distance of meshes or point clouds (evaluation/dtu_eval.py on the GPU)")
    ap.add_argument("--outdir", type=str, default="./outputs")
    ap.add_argument("--scan", type=int, default=1, help="accepted and unused, as in the reference")
    ap.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    ap.add_argument("--dataset_dir", type=str, default="./MVS_Data")
    ap.add_argument("--vis_out_dir", type=str, default=".", help="directory of the error clouds; unused without --write_vis")
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--patch_size", type=float, default=60)
    ap.add_argument("--max_dist", type=float, default=20)
    ap.add_argument("--visualize_threshold", type=float, default=10,
                    help="distance at which an error cloud's ramp reaches full red; unused without --write_vis")
    ap.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the reference's 15 test scans)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the shuffle before thinning")
    ap.add_argument("--mesh_dir", type=str, default=None,
                    help="directory holding scan{N}.ply (default <outdir>/mesh/final; <outdir>/mesh scores the un-cleaned "
                         "meshes that `python -m uforecon_amd.tsdf` writes)")
    ap.add_argument("--write_vis", action="store_true",
                    help="write the error-coloured clouds <vis_out_dir>/vis_<scan:03>_d2s.ply and ..._s2d.ply of every scan")
    args = ap.parse_args(argv)
    if args.write_vis:
        os.makedirs(args.vis_out_dir, exist_ok=True)

    log = logging.getLogger("uforecon_amd.dtu_eval")
    handler = logging.FileHandler(f"{args.outdir}/eval_final.log")
    handler.setFormatter(logging.Formatter("INFO:root:%(message)s"))       # the prefix the reference's log_to_csv.py looks for
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    log.propagate = False
    d2s_l, s2d_l, all_l = [], [], []
    try:
        for scan in args.scans:
            if args.mode == "mesh":
                data = os.path.join(args.mesh_dir or os.path.join(args.outdir, "mesh", "final"), "scan{}.ply".format(scan))
                if not os.path.exists(data):
                    print("mesh not found: {}".format(data))
                    continue
            else:
                data = os.path.join(args.outdir, "pcd", "scan{}.ply".format(scan))
            r = evaluate_scan(data, args.mode, f"{args.dataset_dir}/Points/stl/stl{scan:03}_total.ply",
                              _pick(f"{args.dataset_dir}/ObsMask/ObsMask{scan}_10"), _pick(f"{args.dataset_dir}/ObsMask/Plane{scan}"),
                              density=args.downsample_density, patch=args.patch_size, max_dist=args.max_dist, seed=args.seed,
                              vis_prefix=f"{args.vis_out_dir}/vis_{scan:03}" if args.write_vis else None,
                              vis_dist=args.visualize_threshold)
            print(scan, r["d2s"], r["s2d"], r["overall"])
            log.info("scan: {} | d2s:{} | s2d:{} | all: {}".format(scan, r["d2s"], r["s2d"], r["overall"]))
            d2s_l.append(r["d2s"])
            s2d_l.append(r["s2d"])
            all_l.append(r["overall"])
        print("final result")
        means = [float(np.mean(v)) if v else float("nan") for v in (d2s_l, s2d_l, all_l)]
        print(*means)
        log.info("all | d2s: {} | s2d: {} | all: {}".format(*means))
    finally:
        log.removeHandler(handler)
        handler.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
