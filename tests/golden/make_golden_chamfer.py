"""Writes tests/golden/chamfer_mesh.npz and chamfer_pcd.npz: inputs and recorded results OF THE REFERENCE SCRIPT
evaluation/dtu_eval.py, run unmodified through runpy (its globals are the record).  Run only where the reference tree
exists:  python tests/golden/make_golden_chamfer.py /path/to/reference

Three shims, all in this harness and none in the reference: a stub ``open3d`` whose readers hand back the fixture's arrays
(open3d is not a dependency here); ``numpy.__all__`` without max / min / round / abs while the script runs (numpy 2 exports
them, and the script's ``from numpy import *`` would then shadow the builtins it calls); ``numpy.random.default_rng``
replaced by a seeded one (the script shuffles with an unseeded generator).  The script's scan list is hard-coded, so the
fixture is "scan24"; in --mode pcd the script does not skip missing scans, so the stub ends the run at the second one after
keeping the globals of the first.

Only data is stored: inputs, masks (packbits), the two distance arrays, the means, and sha256 digests of the intermediate
clouds (they follow from the inputs and the masks)."""
import hashlib
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def sphere_mesh(nlat=40, nlon=80, radius=12.0, centre=(3.0, -2.0, 1.0)):
    th = np.pi * np.arange(1, nlat) / nlat
    ph = 2 * np.pi * np.arange(nlon) / nlon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.cos(th)[:, None] * np.ones(nlon)[None]], -1).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    f = []
    last = len(verts) - 1
    for j in range(nlon):
        k = (j + 1) % nlon
        f.append([0, 1 + j, 1 + k])
        f.append([last, 1 + (nlat - 2) * nlon + k, 1 + (nlat - 2) * nlon + j])
        for i in range(nlat - 2):
            a, b = 1 + i * nlon + j, 1 + i * nlon + k
            c, d = a + nlon, b + nlon
            f += [[a, c, b], [b, c, d]]
    faces = np.asarray(f, np.int32)
    keep = verts[faces].mean(1)[:, 0] - centre[0] <= 11.0            # a hole in the data
    faces = faces[keep]
    tiny = verts[100] + np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]]) + 0.3
    faces = np.concatenate([faces, [[5, 5, 9]], [[len(verts), len(verts) + 1, len(verts) + 2]]]).astype(np.int32)
    return np.concatenate([verts, tiny]), faces


def ground_truth(n, seed, radius=12.15, centre=(3.0, -2.0, 1.0), noise=0.05):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * radius + rng.normal(size=(n, 3)) * noise + np.asarray(centre)
    return p[d[:, 1] <= 0.95].astype(np.float32)                     # a hole in the ground truth


def scene():
    BB = np.array([[-6, -20, -17], [21, 17, 21]], np.float64)
    ObsMask = np.zeros((25, 37, 38), np.uint8)
    ObsMask[:, 5:-4, :30] = 1
    ObsMask[:9, :, :12] = 0
    return dict(BB=BB, Res=np.float64(1.0), ObsMask=ObsMask, P=np.array([0, 0.1, 1, 6], np.float64))


def run_reference(ref_root, mode, fixture, scene_, flags, seed):
    """dtu_eval.py on a temporary tree; returns the script's globals."""
    from scipy.io import savemat

    captured = {}

    class _Stop(Exception):
        pass

    class _Geom:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    def read_triangle_mesh(path):
        return _Geom(vertices=fixture["verts"].copy(), triangles=fixture["faces"].copy())

    def read_point_cloud(path):
        if os.path.basename(path).startswith("stl"):
            return _Geom(points=fixture["gt"].astype(np.float64))
        if "scan24." not in path:
            captured.update(sys._getframe(1).f_globals)
            raise _Stop
        return _Geom(points=fixture["pcd"].astype(np.float64))

    o3d = types.ModuleType("open3d")
    o3d.io = types.SimpleNamespace(read_triangle_mesh=read_triangle_mesh, read_point_cloud=read_point_cloud)
    with tempfile.TemporaryDirectory() as tmp:
        out, data = os.path.join(tmp, "out"), os.path.join(tmp, "data")
        os.makedirs(os.path.join(out, "mesh", "final"))
        os.makedirs(os.path.join(data, "ObsMask"))
        open(os.path.join(out, "mesh", "final", "scan24.ply"), "w").close()
        savemat(os.path.join(data, "ObsMask", "ObsMask24_10.mat"),
                dict(ObsMask=scene_["ObsMask"], BB=scene_["BB"], Res=scene_["Res"]))
        savemat(os.path.join(data, "ObsMask", "Plane24.mat"), dict(P=scene_["P"].reshape(4, 1)))
        saved = dict(argv=sys.argv, all=np.__all__, rng=np.random.default_rng, o3d=sys.modules.get("open3d"))
        sys.argv = ["dtu_eval.py", "--outdir", out, "--mode", mode, "--dataset_dir", data] + flags
        np.__all__ = [n for n in np.__all__ if n not in ("max", "min", "round", "abs")]
        np.random.default_rng = lambda *a: saved["rng"](seed)
        sys.modules["open3d"] = o3d
        try:
            g = runpy.run_path(os.path.join(ref_root, "evaluation", "dtu_eval.py"), run_name="__main__")
        except _Stop:
            g = captured
        finally:
            sys.argv, np.__all__, np.random.default_rng = saved["argv"], saved["all"], saved["rng"]
            if saved["o3d"] is None:
                del sys.modules["open3d"]
            else:
                sys.modules["open3d"] = saved["o3d"]
        log = open(os.path.join(out, "eval_final.log")).read() if os.path.exists(os.path.join(out, "eval_final.log")) else ""
    return g, log


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def share(mask):
    return 1.0 - float(np.mean(mask))


def record(name, mode, fixture, scene_, g, log, density, patch, max_dist, seed):
    mask, inbound, grid_inbound, in_obs, above = (np.asarray(g[k]) for k in ("mask", "inbound", "grid_inbound", "in_obs", "above"))
    d2s, s2d = g["dist_d2s"][:, 0], g["dist_s2d"][:, 0]
    # every branch does work
    assert share(mask) >= 0.15, share(mask)
    assert share(inbound) >= 0.02 and share(grid_inbound) >= 0.02 and share(in_obs) >= 0.02, (share(inbound), share(grid_inbound), share(in_obs))
    assert share(above) >= 0.10, share(above)
    assert np.mean(d2s >= max_dist) >= 0.01 and np.mean(s2d >= max_dist) >= 0.01
    extra = {}
    if mode == "mesh":
        tv = fixture["verts"][fixture["faces"]]
        v1, v2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
        area2 = np.linalg.norm(np.cross(v1, v2), axis=-1)
        assert (area2 == 0).sum() >= 1 and (g["n1"] == 0).sum() >= 1
        extra = dict(verts=fixture["verts"], faces=fixture["faces"], n_new=np.int64(len(g["new_pts"])),
                     sha_unshuffled=digest(np.concatenate([g["vertices"], g["new_pts"]])))
    else:
        p = fixture["pcd"]
        assert len(np.unique(p, axis=0)) < len(p), "no duplicate points"
        extra = dict(pcd=p)
    print(f"{name}: {len(mask)} points, thinning -{share(mask):.1%}, box -{share(inbound):.1%}, grid -{share(grid_inbound):.1%}, "
          f"ObsMask -{share(in_obs):.1%}, plane -{share(above):.1%}, d2s beyond {np.mean(d2s >= max_dist):.1%}, s2d beyond "
          f"{np.mean(s2d >= max_dist):.1%}; d2s {g['mean_d2s']!r} s2d {g['mean_s2d']!r}")
    np.savez_compressed(
        os.path.join(HERE, f"chamfer_{name}.npz"), mode=mode, gt=fixture["gt"], ObsMask=np.packbits(scene_["ObsMask"]),
        ObsMask_shape=np.asarray(scene_["ObsMask"].shape), BB=scene_["BB"], Res=scene_["Res"], P=scene_["P"],
        density=np.float64(density), patch=np.float64(patch), max_dist=np.float64(max_dist), seed=np.int64(seed),
        n_points=np.int64(len(mask)), thin_mask=np.packbits(mask), inbound=np.packbits(inbound),
        grid_inbound=np.packbits(grid_inbound), in_obs=np.packbits(in_obs), above=np.packbits(above),
        n_inbound=np.int64(len(inbound)), n_grid_inbound=np.int64(len(grid_inbound)), n_in_obs=np.int64(len(in_obs)),
        dist_d2s=d2s, dist_s2d=s2d, mean_d2s=np.float64(g["mean_d2s"]), mean_s2d=np.float64(g["mean_s2d"]),
        sha_data_pcd=digest(g["data_pcd"]), sha_data_down=digest(g["data_down"]), sha_data_in=digest(g["data_in"]),
        sha_data_in_obs=digest(g["data_in_obs"]), sha_stl_above=digest(g["stl_above"]), log=log, **extra)


def main(ref_root):
    sc = scene()
    density, patch, max_dist = 0.2, 2.0, 1.0
    flags = ["--patch_size", str(patch), "--max_dist", str(max_dist), "--downsample_density", str(density)]
    verts, faces = sphere_mesh()
    fx = dict(verts=verts, faces=faces, gt=ground_truth(36000, 1))
    g, log = run_reference(ref_root, "mesh", fx, sc, flags, seed=7)
    record("mesh", "mesh", fx, sc, g, log, density, patch, max_dist, 7)

    rng = np.random.default_rng(5)
    d = rng.normal(size=(26000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pcd = (d * 12.0 + rng.normal(size=d.shape) * 0.03 + np.array([3.0, -2.0, 1.0]))[d[:, 0] <= 0.9].astype(np.float32)
    pcd = np.concatenate([pcd, pcd[rng.integers(0, len(pcd), 400)]])           # exact duplicates
    fx = dict(pcd=pcd, gt=ground_truth(30000, 2))
    g, log = run_reference(ref_root, "pcd", fx, sc, flags, seed=11)
    record("pcd", "pcd", fx, sc, g, log, density, patch, max_dist, 11)


if __name__ == "__main__":
    main(sys.argv[1])
