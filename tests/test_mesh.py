"""Meshes from the fused TSDF volume: the marching-cubes case table, its numpy restatement (tests/mcubes_ref.py), the C
ABI's argument checks and the PLY writers (CPU); the HIP kernel against the restatement bit for bit, TSDFVolume.get_mesh /
get_point_cloud and save_tsdf (GPU)."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mcubes_ref as R
from uforecon_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(_lib.LIB_PATH):
        from uforecon_amd.build import build_library

        build_library(verbose=False)
    return ops.marching_cubes_table()


def random_volume(seed, n=24):
    """uniform (-1,1) values on an n^3 interior, a positive (above) border: every surface is closed."""
    rng = np.random.default_rng(seed)
    vol = np.ones((n + 2,) * 3, np.float32)
    vol[1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, (n,) * 3).astype(np.float32)
    return vol


def _grid(n):
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing="ij"), -1)


def sphere_volume(n=32, r=10.0, c=15.3):
    return (np.linalg.norm(_grid(n) - np.float32(c), axis=-1) - np.float32(r)).astype(np.float32)


def torus_volume(n=32, R_=9.0, r=3.5, c=15.5):
    p = _grid(n) - np.float32(c)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - np.float32(R_)
    return (np.sqrt(q ** 2 + p[..., 2] ** 2) - np.float32(r)).astype(np.float32)


def mesh_topology(verts, faces):
    """Asserts a closed, consistently oriented 2-manifold without degenerate or unused vertices; returns V - E + F."""
    f = np.asarray(faces, np.int64)
    assert len(f) > 0
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    d_keys, d_counts = np.unique(directed, axis=0, return_counts=True)
    assert (d_counts == 1).all(), "a directed edge appears twice: not consistently oriented"
    und = np.sort(directed, axis=1)
    u_keys, u_counts = np.unique(und, axis=0, return_counts=True)
    assert (u_counts == 2).all(), collections.Counter(u_counts.tolist())
    assert np.array_equal(np.unique(f), np.arange(len(verts))), "a vertex is not referenced"
    return len(verts) - len(u_keys) + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------ CPU: the table and the restatement
def test_table_matches_its_generator(table):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_mcubes_table as G

    assert table.shape == (256, 16) and table.dtype == np.int8
    tris = G.build_table()
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri]
        assert list(table[case]) == flat + [-1] * (16 - len(flat)), case
    hdr = open(os.path.join(ROOT, "uforecon_amd", "csrc", "mcubes_table.h")).read()
    assert hdr == G.emit_header(tris), "mcubes_table.h is stale: run tools/gen_mcubes_table.py"
    assert table[0].max() == -1 and table[255].max() == -1
    assert ((table >= 0).sum(1) % 3 == 0).all()


@pytest.mark.parametrize("seed", range(4))
def test_random_volumes_give_closed_oriented_manifolds(table, seed):
    vol = random_volume(seed)
    verts, faces, normals = R.marching_cubes(vol, table)
    mesh_topology(verts, faces)


def test_random_volumes_reach_every_case():
    seen = set()
    for seed in range(4):
        seen |= set(np.unique(R.cube_cases(random_volume(seed))).tolist())
    assert seen == set(range(256))


def test_sphere_euler_volume_and_winding(table):
    r = 10.0
    verts, faces, normals = R.marching_cubes(sphere_volume(r=r), table)
    assert mesh_topology(verts, faces) == 2
    vol = signed_volume(verts, faces)
    exact = 4.0 / 3.0 * np.pi * r ** 3
    assert vol > 0 and abs(vol - exact) < 0.01 * exact, (vol, exact)
    # normals point outwards (+grad f) and agree with the faces' right-hand normals
    v = verts.astype(np.float64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    vn = normals[faces].astype(np.float64).sum(1)
    assert (np.einsum("ij,ij->i", fn, vn) > 0).mean() > 0.99
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)


def test_torus_euler(table):
    verts, faces, _ = R.marching_cubes(torus_volume(), table)
    assert mesh_topology(verts, faces) == 0


def test_vertex_set_equals_a_per_axis_edge_scan():
    """The restatement's vertex list against an independent computation: every axis' crossings found on slices of the
    volume, merged in (voxel linear index, axis) order."""
    for vol in (random_volume(7, 12), sphere_volume(20, 6.0, 9.7), torus_volume(24, 7.0, 2.5, 11.5)):
        verts, _, _, _ = R.vertices(vol)
        keys, pos = [], []
        X, Y, Z = vol.shape
        for a in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[a], hi[a] = slice(0, -1), slice(1, None)
            fa, fb = vol[tuple(lo)], vol[tuple(hi)]
            cross = (fa < 0) != (fb < 0)
            ix, iy, iz = np.nonzero(cross)
            t = (np.float32(0) - fa[cross]) / (fb[cross] - fa[cross])
            p = np.stack([ix, iy, iz], 1).astype(np.float32)
            p[:, a] = p[:, a] + t
            keys.append(((ix * Y + iy) * Z + iz) * 3 + a)
            pos.append(p)
        order = np.argsort(np.concatenate(keys), kind="stable")
        assert np.array_equal(verts, np.concatenate(pos)[order])


# ------------------------------------------------------------------ CPU: the C ABI's argument checks
def test_abi_rejects_bad_arguments(table):
    lib = _lib.load()
    fake = C.c_void_p(256)            # never dereferenced: validation returns before any device work
    counts = (C.c_int32 * 2)()
    dim = (C.c_int32 * 3)(8, 1, 8)
    assert lib.ufr_marching_cubes_workspace_bytes(dim) == 0
    assert lib.ufr_marching_cubes_count(fake, dim, 0.0, fake, 1 << 20, counts, None) < 0
    assert b"ufr_marching_cubes_count" in lib.ufr_last_error() and b"8x1x8" in lib.ufr_last_error()
    dim = (C.c_int32 * 3)(8, 9, 10)
    need = lib.ufr_marching_cubes_workspace_bytes(dim)
    assert need >= 4 * 8 * 9 * 10
    assert lib.ufr_marching_cubes_count(None, dim, 0.0, fake, need, counts, None) < 0
    assert b"ufr_marching_cubes_count" in lib.ufr_last_error() and b"null" in lib.ufr_last_error()
    assert lib.ufr_marching_cubes_count(fake, dim, 0.0, fake, need, None, None) < 0
    assert b"null" in lib.ufr_last_error()
    assert lib.ufr_marching_cubes_count(fake, dim, 0.0, fake, need - 1, counts, None) == -3
    assert b"ufr_marching_cubes_count" in lib.ufr_last_error() and b"workspace" in lib.ufr_last_error()
    assert lib.ufr_marching_cubes_emit(fake, dim, 0.0, fake, need - 1, fake, fake, fake, 4, 4, None) == -3
    assert b"ufr_marching_cubes_emit" in lib.ufr_last_error()
    assert lib.ufr_marching_cubes_emit(fake, dim, 0.0, fake, need, None, fake, fake, 4, 4, None) < 0
    assert b"ufr_marching_cubes_emit" in lib.ufr_last_error() and b"null" in lib.ufr_last_error()
    assert lib.ufr_marching_cubes_emit(fake, None, 0.0, fake, need, fake, fake, fake, 4, 4, None) < 0
    assert lib.ufr_marching_cubes_table(None, 4096) < 0
    assert b"ufr_marching_cubes_table" in lib.ufr_last_error()
    out = (C.c_int8 * 100)()
    assert lib.ufr_marching_cubes_table(out, 100) < 0


# ------------------------------------------------------------------ CPU: PLY files
MESH_HEADER = ["ply", "format ascii 1.0", "element vertex {V}", "property float x", "property float y", "property float z",
               "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
               "property uchar blue", "element face {F}", "property list uchar int vertex_index", "end_header"]
PC_HEADER = ["ply", "format ascii 1.0", "element vertex {V}", "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue", "end_header"]


def read_ascii_ply(path):
    """(header lines, vertex rows as float64 (V, k), face rows as int64 (F, 4) or None)."""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    header = lines[:end + 1]
    counts = {l.split()[1]: int(l.split()[2]) for l in header if l.startswith("element")}
    body = lines[end + 1:]
    assert body[-1] == ""
    V, F = counts["vertex"], counts.get("face", 0)
    assert len(body) == V + F + 1
    verts = np.array([[float(x) for x in l.split()] for l in body[:V]]) if V else np.zeros((0, 0))
    faces = None
    if "face" in counts:
        faces = np.array([[int(x) for x in l.split()] for l in body[V:V + F]], np.int64) if F else np.zeros((0, 4), np.int64)
    return header, verts, faces


def test_meshwrite_pcwrite_round_trip(tmp_path, table):
    from uforecon_amd import tsdf as H

    verts, faces, norms = R.marching_cubes(sphere_volume(16, 5.0, 7.4), table)
    verts = verts * np.float32(0.0123) + np.array([-0.5, 0.25, 1000.125], np.float32)
    rng = np.random.default_rng(0)
    colors = rng.integers(0, 256, (len(verts), 3)).astype(np.uint8)
    H.meshwrite(str(tmp_path / "m.ply"), verts, faces, norms, colors)
    header, v, f = read_ascii_ply(str(tmp_path / "m.ply"))
    assert header == [h.format(V=len(verts), F=len(faces)) for h in MESH_HEADER]
    assert np.abs(v[:, :3] - verts).max() <= 5e-7 + 1e-7 * np.abs(verts).max()
    assert np.abs(v[:, 3:6] - norms).max() <= 5e-7
    assert np.array_equal(v[:, 6:], colors)
    assert (f[:, 0] == 3).all() and np.array_equal(f[:, 1:], faces)
    # one line is exactly what the reference's per-vertex "%" formatting gives
    with open(tmp_path / "m.ply") as fh:
        lines = fh.read().split("\n")
    i = len(MESH_HEADER) + 3
    assert lines[i] == "%f %f %f %f %f %f %d %d %d" % (*verts[3], *norms[3], *colors[3])
    assert lines[len(MESH_HEADER) + len(verts) + 2] == "3 %d %d %d" % tuple(faces[2])

    pc = np.hstack([verts, colors])
    H.pcwrite(str(tmp_path / "p.ply"), pc)
    header, v, f = read_ascii_ply(str(tmp_path / "p.ply"))
    assert header == [h.format(V=len(verts)) for h in PC_HEADER] and f is None
    assert np.abs(v[:, :3] - verts).max() <= 5e-7 + 1e-7 * np.abs(verts).max()
    assert np.array_equal(v[:, 3:], colors)

    H.meshwrite(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32),
                np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    header, v, f = read_ascii_ply(str(tmp_path / "e.ply"))
    assert header == [h.format(V=0, F=0) for h in MESH_HEADER] and len(v) == 0 and len(f) == 0


# ------------------------------------------------------------------ GPU: the kernel against the restatement
def _gpu_mc(vol, level=0.0):
    import torch

    v = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    verts, faces, normals = ops.marching_cubes(v, level)
    torch.cuda.synchronize()
    return verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy()


def _assert_same(vol, table, level=0.0):
    verts, faces, normals = _gpu_mc(vol, level)
    rv, rf, rn = R.marching_cubes(vol, table, level)
    assert verts.shape == rv.shape and faces.shape == rf.shape
    assert np.array_equal(verts, rv)
    assert np.array_equal(faces, rf)
    assert np.abs(normals - rn).max() <= 1e-6
    return verts, faces


def _big_volume():
    """10.3 M voxels, no dim a multiple of the 4096-voxel tile or of 64: two overlapping blobs and a wavy sheet."""
    X, Y, Z = 301, 211, 163
    x = np.arange(X, dtype=np.float32)[:, None, None]
    y = np.arange(Y, dtype=np.float32)[None, :, None]
    z = np.arange(Z, dtype=np.float32)[None, None, :]
    d1 = np.sqrt((x - 90) ** 2 + (y - 100) ** 2 + (z - 80) ** 2) - 60
    d2 = np.sqrt((x - 180) ** 2 + (y - 110) ** 2 + (z - 70) ** 2) - 45
    sheet = (x - 250 - 12 * np.sin(y / 9.0) * np.cos(z / 7.0))
    return np.minimum(np.minimum(d1, d2), sheet).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere3", "sphere5_holes"])
def test_kernel_matches_restatement_on_golden_tsdf(table, name):
    g = np.load(os.path.join(HERE, "golden", f"tsdf_{name}.npz"))
    verts, faces = _assert_same(g["tsdf"], table)
    assert len(faces) > 100


@pytest.mark.gpu
def test_kernel_matches_restatement_on_synthetic_volumes(table):
    for seed in range(4):
        _assert_same(random_volume(seed), table)
    _assert_same(sphere_volume(), table)
    _assert_same(torus_volume(), table)
    q = np.round(random_volume(11, 20) * 2) / 2          # quantised: many exact zeros (zero = not below)
    assert (q == 0).sum() > 1000
    _assert_same(q.astype(np.float32), table)
    _assert_same(sphere_volume(), table, level=0.75)       # a non-zero iso-level
    _assert_same(np.random.default_rng(3).uniform(-1, 1, (2, 3, 70)).astype(np.float32), table)   # minimal dims, open


@pytest.mark.gpu
def test_kernel_matches_restatement_on_a_large_non_cubic_volume(table):
    vol = _big_volume()
    assert vol.size >= 10 ** 7
    verts, faces = _assert_same(vol, table)
    assert len(faces) > 10 ** 5


@pytest.mark.gpu
def test_kernel_is_deterministic_and_empty_volumes_give_empty_meshes():
    vol = _big_volume()
    a = _gpu_mc(vol)
    b = _gpu_mc(vol)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    v, f, n = _gpu_mc(np.ones((17, 9, 33), np.float32))
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    assert v.dtype == np.float32 and f.dtype == np.int32


# ------------------------------------------------------------------ GPU: TSDFVolume.get_mesh, save_tsdf
def _fused(name, integrate_color):
    from uforecon_amd import tsdf as H
    from uforecon_amd.scene import make_tsdf_case

    c = make_tsdf_case(name)
    vol = H.fuse_depth_maps(c["depths"], c["intrinsics"], [np.linalg.inv(P) for P in c["poses"]],
                            voxel_size=c["voxel_size"], margin=c["margin"], colors=c["colors"],
                            integrate_color=integrate_color)
    return c, vol


@pytest.mark.gpu
def test_get_mesh_world_coordinates_colours_and_surface(table):
    c, vol = _fused("sphere3", integrate_color=True)
    verts, faces, norms, colors = vol.get_mesh()
    tsdf_vol, color_vol, weight_vol = vol.get_volume()
    rv, rf, rn = R.marching_cubes(tsdf_vol, table)
    assert np.array_equal(faces, rf) and np.abs(norms - rn).max() <= 1e-6
    assert verts.dtype == np.float32 and np.array_equal(verts, rv * vol._voxel_size + vol._vol_origin)
    # the reference's colour formula (tsdf_fusion.py:347-355) on the host copy of the volume
    ind = np.round(rv).astype(int)
    rgb = color_vol[ind[:, 0], ind[:, 1], ind[:, 2]]
    cb = np.floor(rgb / vol._color_const)
    cg = np.floor((rgb - cb * vol._color_const) / 256)
    cr = rgb - cb * vol._color_const - cg * 256
    ref_colors = np.floor(np.asarray([cr, cg, cb])).T.astype(np.uint8)
    assert colors.dtype == np.uint8 and np.array_equal(colors, ref_colors)
    assert len(np.unique(colors, axis=0)) > 50
    # the fused surface is the sphere of radius 0.8, where both edge ends were observed
    vox, axis = np.nonzero(((R.crossing_mask(tsdf_vol)[..., None] >> np.arange(3, dtype=np.uint8)) & 1).reshape(-1, 3))
    p = np.stack(np.unravel_index(vox, tsdf_vol.shape), 1)
    q = p.copy()
    q[np.arange(len(q)), axis] += 1
    seen = (weight_vol[p[:, 0], p[:, 1], p[:, 2]] > 0) & (weight_vol[q[:, 0], q[:, 1], q[:, 2]] > 0)
    assert seen.sum() > 200
    err = np.abs(np.linalg.norm(verts[seen].astype(np.float64), axis=1) - 0.8)
    assert np.median(err) < 0.25 * c["voxel_size"], np.median(err)
    pc = vol.get_point_cloud()
    assert np.array_equal(pc, np.hstack([verts, colors]))


@pytest.mark.gpu
def test_save_tsdf_writes_mesh_and_point_cloud(tmp_path):
    from uforecon_amd import tsdf as H
    from uforecon_amd.model import save_depth_outputs
    from uforecon_amd.scene import make_tsdf_case

    c = make_tsdf_case("sphere3")
    for i, (d, rgb, K, P) in enumerate(zip(c["depths"], c["colors"], c["intrinsics"], c["poses"])):
        save_depth_outputs(str(tmp_path), "scan7", f"refview{i}", d, rgb, np.linalg.inv(P), K)
    V, F = H.save_tsdf(str(tmp_path), "scan7", voxel_size=c["voxel_size"], margin=c["margin"])
    loaded = [np.load(tmp_path / "depth" / "scan7" / f"refview{i}.npy", allow_pickle=True).item() for i in range(3)]
    ref = H.fuse_depth_maps([d["depth"] for d in loaded], [d["intrinsic"] for d in loaded],
                            [d["extrinsic"] for d in loaded], voxel_size=c["voxel_size"], margin=c["margin"])
    verts, faces, norms, colors = ref.get_mesh()
    assert (V, F) == (len(verts), len(faces)) and F > 100
    header, v, f = read_ascii_ply(str(tmp_path / "mesh" / "scan7.ply"))
    assert header == [h.format(V=V, F=F) for h in MESH_HEADER]
    assert np.array_equal(f[:, 1:], faces) and (v[:, 6:] == 0).all()     # the reference fuses no colour
    header, v, _ = read_ascii_ply(str(tmp_path / "pcd" / "scan7.ply"))
    assert header == [h.format(V=V) for h in PC_HEADER]
    assert np.abs(v[:, :3] - verts).max() < 1e-5

    # the command line of tsdf_fusion.py, on the same tree
    os.remove(tmp_path / "mesh" / "scan7.ply")
    r = subprocess.run([sys.executable, "-m", "uforecon_amd.tsdf", "--root_dir", str(tmp_path), "--voxel_size",
                        str(c["voxel_size"]), "--margin", str(c["margin"])], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert "scan7" in r.stdout
    header, _, f = read_ascii_ply(str(tmp_path / "mesh" / "scan7.ply"))
    assert header[2] == f"element vertex {V}" and np.array_equal(f[:, 1:], faces)
