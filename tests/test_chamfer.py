"""DTU chamfer evaluation (uforecon_amd/dtu_eval.py, csrc/chamfer.hip).

CPU: the numpy restatement (tests/chamfer_ref.py) against recorded outputs of the reference's evaluation/dtu_eval.py
(tests/golden/chamfer_*.npz), its grid versions against the sequential loop and brute force, the PLY reader, the C ABI's
argument checks.  GPU: ops.sample_mesh / thin_points / nn_distance and dtu_eval.chamfer against the restatement: points and
masks exactly, distances within 2 ulp, means within 1e-12 relative; the command line on a tree laid out as the reference
expects."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import chamfer_ref as R
from uforecon_amd import _lib, dtu_eval, ops
from uforecon_amd._lib import UfrError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = ("mesh", "pcd")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def unpack(g, key, n):
    return np.unpackbits(g[key])[:int(n)].astype(bool)


def load_golden(name):
    g = dict(np.load(os.path.join(HERE, "golden", f"chamfer_{name}.npz")))
    shape = tuple(int(v) for v in g["ObsMask_shape"])
    g["obs"] = np.unpackbits(g["ObsMask"])[:int(np.prod(shape))].reshape(shape)
    g["data"] = (g["verts"], g["faces"]) if name == "mesh" else g["pcd"]
    g["kw"] = dict(density=float(g["density"]), patch=float(g["patch"]), max_dist=float(g["max_dist"]), seed=int(g["seed"]))
    return g


_restated = {}


def restated(name):
    """the restatement's run of a golden fixture (grid neighbours: the same results as the loop / brute force, see below)"""
    if name not in _restated:
        g = load_golden(name)
        md = g["kw"]["max_dist"]
        _restated[name] = (g, R.chamfer(g["data"], g["gt"], g["obs"], g["BB"], g["Res"], g["P"], nn=lambda q, f: R.nn_grid(q, f, md),
                                        thin=R.thin_grid, **g["kw"]))
    return _restated[name]


def within_ulp(a, b, n=2):
    return np.abs(a - b) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b)))


def assert_distances(got, want, max_dist):
    """the kernel's contract: equal within 2 ulp wherever the true distance is < max_dist, some value >= max_dist elsewhere"""
    near = want < max_dist
    assert within_ulp(got[near], want[near]).all(), np.abs(got[near] - want[near]).max()
    assert (got[~near] >= max_dist).all()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from uforecon_amd.build import build_library

        build_library(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------ CPU: restatement == the reference's recorded run
@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_matches_the_reference_run(name):
    g, r = restated(name)
    md = g["kw"]["max_dist"]
    if name == "mesh":
        assert len(r["data_pcd_unshuffled"]) == len(g["verts"]) + int(g["n_new"])
        assert digest(r["data_pcd_unshuffled"]) == str(g["sha_unshuffled"])
    assert len(r["data_pcd"]) == int(g["n_points"])
    assert digest(r["data_pcd"]) == str(g["sha_data_pcd"])                      # the shuffle is the seeded permutation
    assert np.array_equal(r["thin_mask"], unpack(g, "thin_mask", g["n_points"]))
    assert np.array_equal(r["inbound"], unpack(g, "inbound", g["n_inbound"]))
    assert np.array_equal(r["grid_inbound"], unpack(g, "grid_inbound", g["n_grid_inbound"]))
    assert np.array_equal(r["in_obs"], unpack(g, "in_obs", g["n_in_obs"]))
    assert np.array_equal(r["above"], unpack(g, "above", len(g["gt"])))
    for k in ("data_in", "data_in_obs", "stl_above"):
        assert digest(r[k]) == str(g["sha_" + k]), k
    assert digest(r["data_pcd"][r["thin_mask"]]) == str(g["sha_data_down"])
    for k in ("dist_d2s", "dist_s2d"):
        assert r[k].shape == g[k].shape
        assert_distances(r[k], g[k], md)
        assert_distances(g[k], np.where(r[k] < md, r[k], np.inf), md)           # ... and the same set is below max_dist
    assert abs(r["d2s"] - float(g["mean_d2s"])) <= 1e-12 * float(g["mean_d2s"])
    assert abs(r["s2d"] - float(g["mean_s2d"])) <= 1e-12 * float(g["mean_s2d"])
    # the fixture exercises every branch (the maker asserts the same on the reference's own arrays)
    assert 1 - r["thin_mask"].mean() >= 0.15 and 1 - r["inbound"].mean() >= 0.02 and 1 - r["grid_inbound"].mean() >= 0.02
    assert 1 - r["in_obs"].mean() >= 0.02 and 1 - r["above"].mean() >= 0.10
    assert (g["dist_d2s"] >= md).mean() >= 0.01 and (g["dist_s2d"] >= md).mean() >= 0.01


def test_golden_mesh_has_degenerate_triangles_and_the_cloud_duplicates():
    g = load_golden("mesh")
    _, info = R.sample_mesh(g["verts"], g["faces"], 0.2, return_counts=True)
    assert (~info["non_zero_area"]).sum() >= 1 and ((info["n1"] == 0) | (info["n2"] == 0)).sum() >= 1
    assert info["per_triangle"].max() >= 5 and (info["per_triangle"] == 0).sum() >= 2
    p = load_golden("pcd")["pcd"]
    assert len(np.unique(p, axis=0)) < len(p)


def _noisy_sphere(n, seed, radius=3.0, noise=0.02):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * radius + rng.normal(size=(n, 3)) * noise + np.array([0.5, -1.0, 2.0])


def test_grid_versions_equal_the_loop_and_brute_force():
    p = _noisy_sphere(5000, 0)
    p = np.concatenate([p, p[:200]])[np.random.default_rng(1).permutation(5200)]            # with duplicates
    for r in (0.1, 0.25):
        assert np.array_equal(R.thin_grid(p, r), R.thin_sequential(p, r))
    lattice = np.stack(np.meshgrid(*[np.arange(8) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3)     # exactly r apart
    lattice = lattice[np.random.default_rng(2).permutation(len(lattice))]
    assert np.array_equal(R.thin_grid(lattice, 0.25), R.thin_sequential(lattice, 0.25))
    q = _noisy_sphere(3000, 3, radius=3.1, noise=0.2)
    ref = _noisy_sphere(4000, 4)
    for md in (0.1, 0.3):
        exact = R.nn_brute(q, ref)
        assert np.array_equal(R.nn_grid(q, ref, md), np.where(exact < md, exact, np.inf))
        assert ((exact < md).mean() > 0.05) and ((exact >= md).mean() > 0.05), (exact < md).mean()


def test_restatement_equals_sklearn():
    skln = pytest.importorskip("sklearn.neighbors")
    p = _noisy_sphere(6000, 5)
    p = np.concatenate([p, p[:100]])
    r = 0.12
    nn_engine = skln.NearestNeighbors(n_neighbors=1, radius=r, algorithm="kd_tree")
    nn_engine.fit(p)
    rnn_idxs = nn_engine.radius_neighbors(p, radius=r, return_distance=False)
    mask = np.ones(p.shape[0], dtype=np.bool_)
    for curr, idxs in enumerate(rnn_idxs):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    assert np.array_equal(R.thin_sequential(p, r), mask) and np.array_equal(R.thin_grid(p, r), mask)
    q = _noisy_sphere(3000, 6, radius=3.2, noise=0.3)
    dist, _ = nn_engine.kneighbors(q, n_neighbors=1, return_distance=True)
    assert within_ulp(R.nn_brute(q, p), dist[:, 0]).all()


# ------------------------------------------------------------------ CPU: PLY reader
def write_binary_ply(path, verts, faces=None, vtype="double", extra=False):
    fmt = {"double": "<f8", "float": "<f4"}[vtype]
    fields = [("x", fmt), ("y", fmt), ("z", fmt)] + ([("red", "u1"), ("nx", "<f4")] if extra else [])
    rec = np.zeros(len(verts), np.dtype(fields))
    for i, a in enumerate("xyz"):
        rec[a] = verts[:, i]
    head = ["ply", "format binary_little_endian 1.0", "comment written by a test", f"element vertex {len(verts)}"]
    head += [f"property {vtype} {a}" for a in "xyz"] + (["property uchar red", "property float nx"] if extra else [])
    body = rec.tobytes()
    if faces is not None:
        head += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
        fr = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        fr["n"] = 3
        fr["v"] = faces
        body += fr.tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\nend_header\n").encode() + body)


def test_ply_reader_round_trips(tmp_path):
    from uforecon_amd import tsdf as H

    g = load_golden("mesh")
    verts, faces = g["verts"].astype(np.float32), g["faces"]
    rng = np.random.default_rng(0)
    norms = rng.normal(size=verts.shape).astype(np.float32)
    colors = rng.integers(0, 256, verts.shape).astype(np.uint8)
    H.meshwrite(str(tmp_path / "m.ply"), verts, faces, norms, colors)
    v, f = dtu_eval.read_ply(str(tmp_path / "m.ply"))
    assert v.dtype == np.float64 and f.dtype == np.int32 and np.array_equal(f, faces)
    assert np.array_equal(v, np.array([[float("%f" % x) for x in row] for row in verts]))     # the text, read as float64
    H.pcwrite(str(tmp_path / "p.ply"), np.hstack([verts, colors]))
    v2, f2 = dtu_eval.read_ply(str(tmp_path / "p.ply"))
    assert f2 is None and np.array_equal(v2, v)
    write_binary_ply(str(tmp_path / "b.ply"), g["verts"], faces, "double")
    v, f = dtu_eval.read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(v, g["verts"]) and np.array_equal(f, faces)
    write_binary_ply(str(tmp_path / "c.ply"), verts, None, "float", extra=True)
    v, f = dtu_eval.read_ply(str(tmp_path / "c.ply"))
    assert f is None and np.array_equal(v, verts.astype(np.float64))
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="binary_big_endian"):
        dtu_eval.read_ply(str(tmp_path / "bad.ply"))


def test_observation_arrays_load_from_mat_and_npz(tmp_path):
    sio = pytest.importorskip("scipy.io")
    g = load_golden("mesh")
    sio.savemat(str(tmp_path / "ObsMask24_10.mat"), dict(ObsMask=g["obs"], BB=g["BB"], Res=g["Res"]))
    np.savez(tmp_path / "Plane24.npz", P=g["P"])
    assert dtu_eval._pick(str(tmp_path / "ObsMask24_10")).endswith(".mat") and dtu_eval._pick(str(tmp_path / "Plane24")).endswith(".npz")
    assert dtu_eval._pick(str(tmp_path / "Plane37")).endswith(".mat")                  # the reference's name when neither exists
    obs, bb, res = dtu_eval._load_arrays(str(tmp_path / "ObsMask24_10.mat"), ["ObsMask", "BB", "Res"])
    assert np.array_equal(obs, g["obs"]) and np.array_equal(bb, g["BB"]) and float(res.reshape(-1)[0]) == float(g["Res"])
    (plane,) = dtu_eval._load_arrays(str(tmp_path / "Plane24.npz"), ["P"])
    assert np.array_equal(plane, g["P"])


# ------------------------------------------------------------------ CPU: the C ABI's argument checks
def test_abi_rejects_bad_arguments(lib):
    fake = C.c_void_p(256)            # never dereferenced: validation returns before any device work
    err = lib.ufr_last_error
    total = C.c_int64(0)
    assert lib.ufr_mesh_sample_workspace_bytes(0) == 0 and lib.ufr_mesh_sample_workspace_bytes(2 ** 31) == 0
    need = lib.ufr_mesh_sample_workspace_bytes(1000)
    assert need >= 8 * 1000
    assert lib.ufr_mesh_sample_count(None, fake, 10, 1000, 0.2, fake, need, C.byref(total), None) < 0
    assert b"ufr_mesh_sample_count" in err() and b"null" in err()
    assert lib.ufr_mesh_sample_count(fake, fake, 10, 1000, 0.2, fake, need, None, None) < 0
    assert b"ufr_mesh_sample_count" in err() and b"null" in err()
    assert lib.ufr_mesh_sample_count(fake, fake, 10, 0, 0.2, fake, need, C.byref(total), None) < 0
    assert b"ufr_mesh_sample_count" in err() and b"F 0" in err()
    assert lib.ufr_mesh_sample_count(fake, fake, 10, 1000, 0.0, fake, need, C.byref(total), None) < 0
    assert b"density" in err()
    assert lib.ufr_mesh_sample_count(fake, fake, 10, 1000, 0.2, fake, need - 1, C.byref(total), None) == -3
    assert b"ufr_mesh_sample_count" in err() and b"workspace" in err()
    assert lib.ufr_mesh_sample_emit(fake, fake, 10, 1000, 0.2, fake, need - 1, fake, 5, None) == -3
    assert b"ufr_mesh_sample_emit" in err()
    assert lib.ufr_mesh_sample_emit(fake, fake, 10, 1000, 0.2, fake, need, None, 5, None) < 0
    assert b"ufr_mesh_sample_emit" in err() and b"null" in err()
    assert lib.ufr_mesh_sample_emit(fake, fake, 10, 1000, 0.2, fake, need, fake, -1, None) < 0
    assert b"capacity" in err()

    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.ufr_points_cell_keys(None, 5, origin, 1.0, fake, None) < 0
    assert b"ufr_points_cell_keys" in err() and b"null" in err()
    assert lib.ufr_points_cell_keys(fake, 0, origin, 1.0, fake, None) < 0
    assert b"ufr_points_cell_keys" in err() and b"n 0" in err()
    assert lib.ufr_points_cell_keys(fake, 5, origin, 0.0, fake, None) < 0
    assert b"cell" in err()

    rounds = C.c_int32(0)
    assert lib.ufr_points_thin_workspace_bytes(0) == 0
    need = lib.ufr_points_thin_workspace_bytes(100)
    assert need >= 4
    assert lib.ufr_points_thin(fake, fake, None, 100, 0.2, fake, fake, need, C.byref(rounds), None) < 0
    assert b"ufr_points_thin" in err() and b"null" in err()
    assert lib.ufr_points_thin(fake, fake, fake, -3, 0.2, fake, fake, need, C.byref(rounds), None) < 0
    assert b"ufr_points_thin" in err() and b"n -3" in err()
    assert lib.ufr_points_thin(fake, fake, fake, 100, -1.0, fake, fake, need, C.byref(rounds), None) < 0
    assert b"radius" in err()
    assert lib.ufr_points_thin(fake, fake, fake, 100, 0.2, fake, fake, need - 1, C.byref(rounds), None) == -3
    assert b"ufr_points_thin" in err() and b"workspace" in err()

    assert lib.ufr_points_nn_dist_workspace_bytes(0) == 0
    need = lib.ufr_points_nn_dist_workspace_bytes(1000)
    assert need >= 16 * 4
    assert lib.ufr_points_nn_dist(fake, 1000, None, fake, 10, origin, 1.0, 20.0, fake, None, fake, need, None) < 0
    assert b"ufr_points_nn_dist" in err() and b"null" in err()
    assert lib.ufr_points_nn_dist(fake, 1000, fake, fake, 0, origin, 1.0, 20.0, fake, None, fake, need, None) < 0
    assert b"ufr_points_nn_dist" in err() and b"nr 0" in err()
    assert lib.ufr_points_nn_dist(fake, 0, fake, fake, 10, origin, 1.0, 20.0, fake, None, fake, need, None) < 0
    assert b"nq 0" in err()
    assert lib.ufr_points_nn_dist(fake, 1000, fake, fake, 10, origin, 1.0, 0.0, fake, None, fake, need, None) < 0
    assert b"max_dist" in err()
    assert lib.ufr_points_nn_dist(fake, 1000, fake, fake, 10, origin, 1.0, 20.0, fake, None, fake, need - 1, None) == -3
    assert b"ufr_points_nn_dist" in err() and b"workspace" in err()


def test_ops_refuse_host_tensors_and_wrong_dtypes(lib):
    import torch

    p = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(UfrError, match="GPU"):
        ops.thin_points(p, 0.2)
    with pytest.raises(UfrError, match="GPU"):
        ops.nn_distance(p, p, 1.0)
    with pytest.raises(UfrError, match="GPU"):
        ops.sample_mesh(p, torch.zeros((1, 3), dtype=torch.int32), 0.2)


# ------------------------------------------------------------------ GPU helpers
def _cuda(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype) if dtype is not None else t.cuda()


def gpu_sample(verts, faces, density):
    import torch

    out = ops.sample_mesh(_cuda(verts, torch.float64), _cuda(faces, torch.int32), density)
    return out.cpu().numpy()


def gpu_thin(points, r):
    import torch

    keep, rounds = ops.thin_points(_cuda(points, torch.float64), r, return_rounds=True)
    return keep.cpu().numpy(), rounds


def gpu_nn(query, ref, max_dist):
    import torch

    d, sums = ops.nn_distance(_cuda(query, torch.float64), _cuda(ref, torch.float64), max_dist, return_sums=True)
    return d.cpu().numpy(), sums.cpu().numpy()


def _mc_mesh(n, radius, scale):
    """a marching-cubes mesh of a sphere with a wavy surface, scaled; float64 vertices, int32 faces"""
    import torch

    x = np.arange(n, dtype=np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    c = np.float32(n / 2 - 0.3)
    vol = np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2) - np.float32(radius) + np.float32(0.7) * np.sin(X / 3) * np.cos(Y / 4)
    verts, faces, _ = ops.marching_cubes(torch.from_numpy(vol.astype(np.float32)).cuda())
    return verts.cpu().numpy().astype(np.float64) * scale, faces.cpu().numpy()


# ------------------------------------------------------------------ GPU: mesh sampling
@pytest.mark.gpu
def test_sample_mesh_equals_restatement_on_the_golden_mesh():
    g, r = restated("mesh")
    got = gpu_sample(g["verts"], g["faces"], g["kw"]["density"])
    assert got.shape == r["data_pcd_unshuffled"].shape
    assert np.array_equal(got, r["data_pcd_unshuffled"])
    assert digest(got) == str(g["sha_unshuffled"])                              # = the reference's own cloud


@pytest.mark.gpu
def test_sample_mesh_equals_restatement_on_marching_cubes_meshes():
    verts, faces = _mc_mesh(32, 10.0, 1.6)
    want, info = R.sample_mesh(verts, faces, 0.2, return_counts=True)
    assert info["per_triangle"].min() == 0 and 30 <= info["per_triangle"].max() <= 80, info["per_triangle"].max()
    got = gpu_sample(verts, faces, 0.2)
    assert got.shape == want.shape and np.array_equal(got, want)
    for density in (0.05, 1.7):                                                 # many samples per triangle; almost none
        want = R.sample_mesh(verts, faces, density)
        got = gpu_sample(verts, faces, density)
        assert got.shape == want.shape and np.array_equal(got, want)


def _jittered_grid(n, seed):
    """an n x n planar grid at unit spacing, every coordinate jittered by up to 0.2, two triangles per cell in shuffled order"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3) + rng.uniform(-0.2, 0.2, (n * n, 3))
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    return verts, faces[rng.permutation(len(faces))].astype(np.int32)


@pytest.mark.gpu
def test_sample_mesh_equals_restatement_past_1024_blocks():
    """more blocks than the totals scan has threads: every scan thread sums several block totals, the last ones none"""
    verts, faces = _jittered_grid(364, 5)
    assert len(faces) == 263_538 and -(-len(faces) // 256) > 1024
    want, info = R.sample_mesh(verts, faces, 0.3, return_counts=True)
    assert info["per_triangle"].min() == 0 and info["per_triangle"].max() >= 8, info["per_triangle"].max()
    got = gpu_sample(verts, faces, 0.3)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
def test_sample_mesh_equals_restatement_on_two_million_points():
    verts, faces = _mc_mesh(96, 40.0, 2.3)
    want = R.sample_mesh(verts, faces, 0.2)
    assert len(want) >= 2_000_000
    got = gpu_sample(verts, faces, 0.2)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(gpu_sample(verts, faces, 0.2), got)


# ------------------------------------------------------------------ GPU: thinning
@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_thin_points_equals_the_reference_on_golden_clouds(name):
    g, r = restated(name)
    keep, rounds = gpu_thin(r["data_pcd"], g["kw"]["density"])
    assert np.array_equal(keep, unpack(g, "thin_mask", g["n_points"]))          # the reference's own mask
    assert 1 <= rounds <= 64
    keep2, _ = gpu_thin(r["data_pcd"], g["kw"]["density"])
    assert np.array_equal(keep, keep2)


@pytest.mark.gpu
def test_thin_points_duplicates_exact_radius_and_adversarial_order():
    lattice = np.stack(np.meshgrid(*[np.arange(12) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3)     # exactly r apart
    rng = np.random.default_rng(0)
    cloud = np.concatenate([lattice, lattice[rng.integers(0, len(lattice), 300)], _noisy_sphere(3000, 1, 1.2, 0.05) + 1.0])
    cloud = cloud[rng.permutation(len(cloud))]
    want = R.thin_sequential(cloud, 0.25)
    keep, _ = gpu_thin(cloud, 0.25)
    assert np.array_equal(keep, want)
    assert 0.05 < want.mean() < 0.6
    keep0, _ = gpu_thin(cloud, 0.0)                                             # radius 0: only exact duplicates go
    assert np.array_equal(keep0, R.thin_sequential(cloud, 0.0)) and keep0.sum() == len(np.unique(cloud, axis=0))
    # points in order along a line, 0.6 r apart: every decision waits for the one before it
    line = np.zeros((3000, 3))
    line[:, 0] = np.arange(3000) * 0.15
    want = R.thin_sequential(line, 0.25)
    keep, rounds = gpu_thin(line, 0.25)
    assert np.array_equal(keep, want) and np.array_equal(keep, np.arange(3000) % 2 == 0)
    assert rounds >= 32
    one, _ = gpu_thin(np.array([[1.0, 2.0, 3.0]]), 0.2)
    assert one.tolist() == [True]


@pytest.mark.gpu
def test_thin_points_equals_restatement_on_two_million_points():
    rng = np.random.default_rng(3)
    cloud = np.concatenate([_noisy_sphere(1_200_000, 4, 52.0, 0.05), _noisy_sphere(900_000, 5, 40.0, 0.3) + 7.0])
    cloud = np.concatenate([cloud, cloud[rng.integers(0, len(cloud), 1000)]])
    cloud = cloud[rng.permutation(len(cloud))]
    assert len(cloud) >= 2_000_000
    want = R.thin_grid(cloud, 0.2)
    keep, rounds = gpu_thin(cloud, 0.2)
    assert (keep != want).sum() == 0
    assert 0.15 < 1 - want.mean() < 0.9 and rounds <= 64
    keep2, _ = gpu_thin(cloud, 0.2)
    assert np.array_equal(keep, keep2)


# ------------------------------------------------------------------ GPU: nearest neighbours
@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_nn_distance_equals_the_reference_on_golden_clouds(name):
    g, r = restated(name)
    md = g["kw"]["max_dist"]
    stl = g["gt"].astype(np.float64)
    for query, ref, key in ((r["data_in_obs"], stl, "dist_d2s"), (r["stl_above"], r["data_in"], "dist_s2d")):
        d, sums = gpu_nn(query, ref, md)
        assert_distances(d, g[key], md)                                         # the reference's own distances
        assert_distances(d, r[key], md)
        near = d < md
        assert sums[1] == near.sum() and abs(sums[0] - d[near].sum()) <= 1e-12 * d[near].sum()
        d2, sums2 = gpu_nn(query, ref, md)
        assert np.array_equal(d, d2) and np.array_equal(sums, sums2)            # run-to-run identical, the sums included
        exact, _ = gpu_nn(query, ref, 1e6)                                      # an unbounded search: every distance exact
        assert within_ulp(exact[:4000], R.nn_brute(query[:4000], ref)).all()


@pytest.mark.gpu
def test_nn_distance_far_queries_single_reference_and_coincident_points():
    ref = _noisy_sphere(50_000, 7)
    rng = np.random.default_rng(8)
    query = _noisy_sphere(20_000, 9, 3.05, 0.1)
    far = rng.choice(len(query), len(query) // 20, replace=False)
    query[far] += rng.choice([-1.0, 1.0], (len(far), 3)) * rng.uniform(40.0, 4000.0, (len(far), 1))
    md = 0.5
    want = R.nn_grid(query, ref, md)
    assert np.isinf(want[far]).all() and (want < md).mean() > 0.9
    d, _ = gpu_nn(query, ref, md)
    assert_distances(d, want, md)
    assert_distances(d[:3000], R.nn_brute(query[:3000], ref), md)
    # one reference point
    d, sums = gpu_nn(query, ref[:1], 3.0)
    exact = R.nn_brute(query, ref[:1])
    assert_distances(d, exact, 3.0)
    assert (exact < 3.0).sum() > 100 and sums[1] == (exact < 3.0).sum()
    # queries that are reference points, and a reference set of identical points
    d, _ = gpu_nn(ref[::7], ref, md)
    assert (d == 0).all()
    d, _ = gpu_nn(query[:100], np.repeat(ref[:1], 500, 0), 3.0)
    assert_distances(d, exact[:100], 3.0)


@pytest.mark.gpu
def test_nn_distance_one_million_by_one_million():
    ref = np.concatenate([_noisy_sphere(600_000, 10, 60.0, 0.05), _noisy_sphere(400_000, 11, 45.0, 0.2) + 5.0])
    query = np.concatenate([_noisy_sphere(600_000, 12, 60.2, 0.1), _noisy_sphere(400_000, 13, 47.0, 1.0) + 5.0])
    md = 0.6
    want = R.nn_grid(query, ref, md)
    assert 0.3 < (want < md).mean() < 0.98
    d, sums = gpu_nn(query, ref, md)
    assert_distances(d, want, md)
    assert sums[1] == (want < md).sum()
    assert abs(sums[0] / sums[1] - want[want < md].mean()) <= 1e-12 * want[want < md].mean()


# ------------------------------------------------------------------ GPU: the whole evaluation
@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_chamfer_equals_the_reference_on_goldens(name):
    g, r = restated(name)
    out = dtu_eval.chamfer(g["data"], g["gt"], g["obs"], g["BB"], g["Res"], g["P"], details=True, **g["kw"])
    assert out["counts"] == r["counts"]
    assert out["counts"]["sampled"] == int(g["n_points"]) and out["counts"]["in_box"] == int(g["n_grid_inbound"])
    assert out["counts"]["in_grid"] == int(g["n_in_obs"]) and out["counts"]["in_obs"] == len(g["dist_d2s"])
    assert out["counts"]["gt_above"] == len(g["dist_s2d"])
    for k in ("thin_mask", "inbound", "grid_inbound", "in_obs", "above"):
        assert np.array_equal(out[k].cpu().numpy(), r[k]), k
    # fp64 sums of < 1e5 positive terms in another order: within 1e-12 relative of the reference's recorded means
    # (measured on an MI355X: 0 to 4.4e-16)
    print(name, "d2s rel err", abs(out["d2s"] / float(g["mean_d2s"]) - 1), "s2d rel err", abs(out["s2d"] / float(g["mean_s2d"]) - 1))
    assert abs(out["d2s"] - float(g["mean_d2s"])) <= 1e-12 * float(g["mean_d2s"])
    assert abs(out["s2d"] - float(g["mean_s2d"])) <= 1e-12 * float(g["mean_s2d"])
    assert out["overall"] == (out["d2s"] + out["s2d"]) / 2
    again = dtu_eval.chamfer(g["data"], g["gt"], g["obs"], g["BB"], g["Res"], g["P"], **g["kw"])
    assert (again["d2s"], again["s2d"]) == (out["d2s"], out["s2d"])


@pytest.mark.gpu
def test_chamfer_of_a_fused_sphere_equals_restatement():
    from uforecon_amd import tsdf as H
    from uforecon_amd.scene import make_tsdf_case

    c = make_tsdf_case("sphere3")
    vol = H.fuse_depth_maps(c["depths"], c["intrinsics"], [np.linalg.inv(P) for P in c["poses"]], voxel_size=c["voxel_size"],
                            margin=c["margin"], colors=c["colors"])
    verts, faces, _, _ = vol.get_mesh()
    assert verts.dtype == np.float32 and len(faces) > 100
    rng = np.random.default_rng(0)
    d = rng.normal(size=(40_000, 3))
    gt = (d / np.linalg.norm(d, axis=1, keepdims=True) * 0.8).astype(np.float32)           # the analytic sphere
    lo = np.floor(verts.min(0).astype(np.float64) - 0.1)
    bb = np.stack([lo, lo + 4.0])
    obs = np.ones((41, 41, 41), np.uint8)
    kw = dict(density=0.02, patch=0.5, max_dist=0.2, seed=3)
    plane = np.array([0.0, 0.0, 1.0, 100.0])
    out = dtu_eval.chamfer((verts, faces), gt, obs, bb, 0.1, plane, **kw)
    r = R.chamfer((verts.astype(np.float64), faces), gt, obs, bb, np.float64(0.1), plane, nn=lambda q, f: R.nn_grid(q, f, 0.2),
                  thin=R.thin_grid, **kw)
    assert out["counts"] == r["counts"] and out["counts"]["in_obs"] > 1000
    print("fused sphere3 chamfer:", out)
    assert abs(out["d2s"] - r["d2s"]) <= 1e-12 * r["d2s"] and abs(out["s2d"] - r["s2d"]) <= 1e-12 * r["s2d"]


@pytest.mark.gpu
def test_command_line_on_a_reference_tree(tmp_path):
    g, _ = restated("mesh")
    out, data = tmp_path / "out", tmp_path / "MVS_Data"
    for d in (out / "mesh" / "final", out / "pcd", data / "ObsMask", data / "Points" / "stl"):
        os.makedirs(d)
    write_binary_ply(str(out / "mesh" / "final" / "scan24.ply"), g["verts"], g["faces"], "double")
    write_binary_ply(str(data / "Points" / "stl" / "stl024_total.ply"), g["gt"], None, "float", extra=True)
    np.savez(data / "ObsMask" / "ObsMask24_10.npz", ObsMask=g["obs"], BB=g["BB"], Res=g["Res"])
    np.savez(data / "ObsMask" / "Plane24.npz", P=g["P"])
    kw = g["kw"]
    cmd = [sys.executable, "-m", "uforecon_amd.dtu_eval", "--outdir", str(out), "--dataset_dir", str(data), "--mode", "mesh",
           "--downsample_density", str(kw["density"]), "--patch_size", str(kw["patch"]), "--max_dist", str(kw["max_dist"]),
           "--seed", str(kw["seed"])]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "mesh not found: {}".format(out / "mesh" / "final" / "scan37.ply") in r.stdout      # the reference's message
    lines = open(out / "eval_final.log").read().split("\n")
    num = r"(\d+\.\d+(?:e-?\d+)?)"
    m = re.fullmatch(rf"INFO:root:scan: 24 \| d2s:{num} \| s2d:{num} \| all: {num}", lines[0])
    assert m, lines
    m2 = re.fullmatch(rf"INFO:root:all \| d2s: {num} \| s2d: {num} \| all: {num}", lines[1])
    assert m2 and m2.groups() == m.groups(), lines
    want = dtu_eval.chamfer(g["data"], g["gt"], g["obs"], g["BB"], g["Res"], g["P"], **kw)
    assert [float(v) for v in m.groups()] == [want["d2s"], want["s2d"], want["overall"]]
    # --mode pcd and --mesh_dir on the same tree; the log is appended to
    write_binary_ply(str(out / "pcd" / "scan24.ply"), load_golden("pcd")["pcd"], None, "float")
    r = subprocess.run(cmd[:7] + ["--mode", "pcd", "--scans", "24", "--max_dist", "1.0", "--patch_size", "2"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    os.rename(out / "mesh" / "final" / "scan24.ply", out / "mesh" / "scan24.ply")
    r = subprocess.run(cmd + ["--mesh_dir", str(out / "mesh"), "--scans", "24"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = open(out / "eval_final.log").read().split("\n")
    assert len(lines) == 7 and lines[4] == lines[0] and lines[2].startswith("INFO:root:scan: 24 | d2s:")
