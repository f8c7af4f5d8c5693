"""Poisson surface reconstruction (uforecon_amd/poisson_mesh.py, csrc/poisson.hip), the parts that need no GPU: the numpy /
scipy restatement (poisson_ref.py) against its own invariants and on the two sphere clouds, the header section against the
ctypes signatures, the host-only grid entry point against the restatement, the command line's flags, and the PLY reader's
normals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poisson_ref as R
from uforecon_amd import _lib, dtu_eval, ops, pcd_filter, poisson_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CENTRE = np.array([0.3, -0.2, 0.1])


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(_lib.LIB_PATH):
        from uforecon_amd.build import build_library

        build_library(verbose=False)
    return ops.marching_cubes_table()


# ------------------------------------------------------------------ splat, matrix, solve
def test_weights_sum_to_one_and_dropped_samples_are_counted():
    P, N = R.sphere_cloud(500, seed=3)
    N[7] = 0.0
    N[11, 1] = np.nan
    ok = R.keep_mask(N)
    assert (~ok).sum() == 2 and not ok[7] and not ok[11]
    P, N = P[ok], N[ok]
    origin, h, dims = R.grid(P, 8, 2)
    V, W = R.splat(P, N, origin, h, dims)
    assert abs(W.sum() - len(P)) <= 1e-12 * len(P)
    for a in range(3):
        assert abs(V[a].sum() - N[:, a].sum()) <= 1e-12 * len(P)
    assert W.min() >= 0.0 and (W[:1].max(), W[-1:].max(), W[:, :1].max(), W[:, :, -1:].max()) == (0.0, 0.0, 0.0, 0.0)   # pad keeps the rim empty


def test_grid_rule_and_refusals():
    P = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.5]])
    origin, h, dims = R.grid(P, 8, 3)
    assert h == 0.25 and origin.tolist() == [-0.75, -0.75, -0.75] and dims.tolist() == [8 + 7, 4 + 7, 2 + 7]
    for bad in (dict(resolution=3), dict(pad=1), dict(resolution=4000, pad=4)):
        with pytest.raises(ValueError):
            R.grid(P, **dict(dict(resolution=8, pad=3), **bad))
    with pytest.raises(ValueError):
        R.grid(np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]), 8, 3)
    with pytest.raises(ValueError):
        R.grid(np.array([[1.0, np.inf, 1.0], [0.0, 1.0, 1.0]]), 8, 3)


def test_matrix_is_symmetric_positive_and_is_the_stencil():
    dims, h = (5, 6, 7), 0.3
    A = R.matrix(dims, h)
    assert abs(A - A.T).max() == 0.0
    p = np.random.default_rng(0).standard_normal(dims)
    q = (A @ p.reshape(-1)).reshape(dims)
    assert np.abs(q - R.laplacian(p, h)).max() <= 1e-12 * np.abs(q).max()
    lam = np.linalg.eigvalsh(A.toarray())
    assert lam.min() > 0.0
    n = max(dims)
    assert lam.max() / lam.min() <= 4 * (n + 1) ** 2 / np.pi ** 2       # the bound the GPU test's tolerance rests on


@pytest.mark.parametrize("dims", [(17, 13, 11), (32, 32, 32)])
def test_fast_diagonalisation_solves_the_matrix(dims):
    b = np.random.default_rng(1).standard_normal(dims)
    h = 0.07
    x = R.solve(b, h)
    res = R.matrix(dims, h) @ x.reshape(-1) + b.reshape(-1)
    assert np.abs(res).max() <= 1e-12 * np.abs(b).max()
    if dims == (17, 13, 11):                                            # the LU is slow beyond this
        assert np.abs(x - R.solve_lu(b, h)).max() <= 1e-12 * np.abs(x).max()


# ------------------------------------------------------------------ the two spheres
def test_full_sphere_lies_within_half_a_cell(table):
    P, N = R.sphere_cloud()
    assert P.shape == (4000, 3)
    out = R.reconstruct(P, N, table, resolution=32, pad=3)
    d = np.abs(np.linalg.norm(out["verts"] - CENTRE, axis=1) - 1.0) / out["h"]
    print("full sphere: worst vertex %.4f h, %d vertices, dims %s" % (d.max(), len(d), out["dims"].tolist()))   # 0.1439 h
    assert len(d) > 1000 and d.max() <= 0.5
    assert out["dropped"] == 0 and out["keep"].all()


def test_partial_sphere_trim_keeps_the_cap_and_removes_the_closure(table):
    P, N = R.sphere_cloud(20000, z_min=-0.3)
    assert len(P) == 12932
    out = R.reconstruct(P, N, table, resolution=32, pad=4, min_density=0.25)
    h = out["h"]
    kept = np.abs(np.linalg.norm(out["verts"] - CENTRE, axis=1) - 1.0) / h
    every = np.abs(np.linalg.norm(out["verts_all"] - CENTRE, axis=1) - 1.0) / h
    above = out["verts_all"][:, 2] - CENTRE[2] > -0.15
    print("partial sphere: worst kept vertex %.4f h, worst untrimmed %.2f h, lost above -0.15: %d" %
          (kept.max(), every.max(), int((above & ~out["keep"]).sum())))            # 1.0521 h, 12.17 h, 0
    assert kept.max() <= 1.5
    assert not (above & ~out["keep"]).any()
    assert every.max() > 5.0
    f = out["faces"]
    assert f.min() >= 0 and f.max() < len(out["verts"]) and np.array_equal(out["verts"], out["verts_all"][out["keep"]])


def test_trim_compacts_and_keeps_order():
    verts = np.arange(15.0).reshape(5, 3)
    faces = np.array([[0, 1, 2], [2, 3, 4], [0, 2, 4], [4, 2, 0]], np.int32)
    v, f, keep = R.trim(verts, faces, np.array([1.0, 0.1, 1.0, 1.0, 1.0]), 0.5)
    assert keep.tolist() == [True, False, True, True, True]
    assert np.array_equal(v, verts[[0, 2, 3, 4]]) and f.tolist() == [[1, 2, 3], [0, 1, 3], [3, 1, 0]]


def test_nearest_colours_tie_goes_to_the_lowest_index():
    pts = np.array([[0.0, 0, 0], [2.0, 0, 0], [2.0, 0, 0], [0.0, 4, 0]])
    col = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]], np.uint8)
    got = R.nearest_colours(np.array([[1.0, 0, 0], [1.9, 0, 0], [0, 3.0, 0]]), pts, col)
    assert got.tolist() == [[1, 1, 1], [2, 2, 2], [4, 4, 4]]


# ------------------------------------------------------------------ header, signatures, the host-only entry point
NEW_SYMBOLS = {"ufr_poisson_grid": 7, "ufr_poisson_splat_keys": 7, "ufr_poisson_splat": 11, "ufr_poisson_divergence": 5,
               "ufr_poisson_laplacian": 5, "ufr_poisson_workspace_bytes": 1, "ufr_poisson_solve": 13,
               "ufr_poisson_sample_workspace_bytes": 1, "ufr_poisson_sample": 11}


def test_header_section_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert hdr.count("/* ---- Poisson surface reconstruction (ABI 507, additive) ----") == 1
    section = hdr[hdr.index("Poisson surface reconstruction (ABI 507, additive)"):]
    section = section[:section.index("void ufr_profile_enable")]
    code = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    found = {}
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code):
        found[name] = len(params.split(","))
        assert _lib.SIGNATURES[name][0] is (C.c_int if res == "int" else C.c_size_t)
    assert found == NEW_SYMBOLS
    for name, n_args in NEW_SYMBOLS.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert "#define UFR_POISSON_MAX_PARTIALS 1024" in code and ops.POISSON_MAX_PARTIALS == 1024
    assert _lib.ABI_VERSION == 507
    from uforecon_amd.build import SOURCES

    assert "poisson.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "uforecon_amd", "csrc", "poisson.hip"))
    assert "neither Open3D nor PoissonRecon was compared" in section
    for name in ("poisson_grid", "poisson_splat", "poisson_divergence", "poisson_laplacian", "poisson_solve", "poisson_workspace_bytes"):
        assert callable(getattr(ops, name))


def _lib_grid(lib, mn, mx, resolution, pad):
    origin, h, dims = (C.c_double * 3)(), C.c_double(0.0), (C.c_int32 * 3)()
    rc = lib.ufr_poisson_grid((C.c_double * 3)(*mn), (C.c_double * 3)(*mx), resolution, pad, origin, C.byref(h), dims)
    return rc, list(origin), h.value, list(dims)


def test_library_grid_equals_the_restatement_and_refuses_without_a_gpu(table):
    lib = _lib.load()
    for seed, (res, pad) in enumerate([(32, 3), (8, 2), (256, 4), (17, 5)]):
        P = np.random.default_rng(seed).standard_normal((50, 3)) * [1.0, 0.37, 2.2]
        origin, h, dims = R.grid(P, res, pad)
        rc, o, hh, d = _lib_grid(lib, P.min(0), P.max(0), res, pad)
        assert rc == 0 and hh == h and o == origin.tolist() and d == dims.tolist()
    err = lib.ufr_last_error
    assert _lib_grid(lib, [0, 0, 0], [1, 1, 1], 3, 4)[0] == -1 and b"resolution 3" in err()
    assert _lib_grid(lib, [0, 0, 0], [1, 1, 1], 8, 1)[0] == -1 and b"pad 1" in err()
    assert _lib_grid(lib, [0, 0, 0], [1, 1, 1], 1300, 4)[0] == -1 and b"2^31" in err()
    assert _lib_grid(lib, [1, 1, 1], [1, 1, 1], 8, 4)[0] == -1 and b"degenerate" in err()
    assert _lib_grid(lib, [0, 0, 0], [1, float("inf"), 1], 8, 4)[0] == -1 and b"not finite" in err()
    assert _lib_grid(lib, [0, float("nan"), 0], [1, 1, 1], 8, 4)[0] == -1 and b"not finite" in err()
    assert _lib_grid(lib, [0, 0, 0], [1, 1, 1], 1200, 4)[0] == 0                       # 1209^3 < 2^31
    # the other entry points refuse before a launch: no GPU is needed to be told so
    fake = C.c_void_p(64)
    dims = (C.c_int32 * 3)(4, 1, 4)
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.ufr_poisson_workspace_bytes(dims) == 0
    assert lib.ufr_poisson_laplacian(fake, dims, 1.0, C.c_void_p(128), None) == -1 and b"4x1x4" in err()
    dims = (C.c_int32 * 3)(4, 4, 4)
    assert lib.ufr_poisson_workspace_bytes(dims) >= 3 * 64 * 8 + 2 * 1024 * 8
    assert lib.ufr_poisson_laplacian(fake, dims, 1.0, fake, None) == -1 and b"aliases" in err()
    assert lib.ufr_poisson_divergence(fake, dims, 0.0, fake, None) == -1 and b"h 0" in err()
    it, res, conv = C.c_int32(), C.c_double(), C.c_int32()
    need = lib.ufr_poisson_workspace_bytes(dims)
    args = (C.byref(it), C.byref(res), C.byref(conv), None)
    assert lib.ufr_poisson_solve(fake, dims, 1.0, 1e-6, 10, 16, fake, fake, need - 1, *args) == -3 and b"workspace" in err()
    assert lib.ufr_poisson_solve(fake, dims, 1.0, 1e-6, 0, 16, fake, fake, need, *args) == -1 and b"max_iter 0" in err()
    assert lib.ufr_poisson_solve(fake, dims, 1.0, -1.0, 10, 16, fake, fake, need, *args) == -1 and b"tol" in err()
    assert lib.ufr_poisson_splat_keys(fake, 0, o3, 1.0, dims, fake, None) == -1 and b"n 0" in err()
    assert lib.ufr_poisson_splat(fake, fake, 5, o3, float("nan"), dims, fake, fake, fake, fake, None) == -1
    assert lib.ufr_poisson_sample(fake, dims, o3, 1.0, fake, 5, fake, None, fake, 0, None) == -3


# ------------------------------------------------------------------ the command line and the reader
def test_parser_flags_and_defaults():
    args = poisson_mesh.make_parser().parse_args(["--out_dir", "x"])
    assert vars(args) == dict(root_dir="./outputs", out_dir="x", scans=None, ply=None, resolution=256, pad=4, tol=1e-6, max_iter=None,
                              min_density=0.0, color=False, normals=0, dataset_dir=None, views=[23, 24, 33])
    args = poisson_mesh.make_parser().parse_args("--root_dir a --out_dir b --scans 24 37 --resolution 128 --pad 3 --tol 1e-8 --max_iter 99 "
                                                 "--min_density 0.5 --color --normals 16 --dataset_dir d --views 1 2 --ply p.ply".split())
    assert (args.scans, args.ply, args.resolution, args.pad, args.tol, args.max_iter) == ([24, 37], ["p.ply"], 128, 3, 1e-8, 99)
    assert (args.min_density, args.color, args.normals, args.dataset_dir, args.views) == (0.5, True, 16, "d", [1, 2])


def test_read_ply_keeps_normals_on_request(tmp_path):
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    nrm = rng.standard_normal((37, 3)).astype(np.float32)
    path = str(tmp_path / "c.ply")
    pcd_filter.write_ply(path, xyz, rgb, nrm)
    v, f, c, n = dtu_eval.read_ply(path, with_colors=True, with_normals=True)
    assert f is None and np.array_equal(v, xyz.astype(np.float64)) and np.array_equal(c, rgb)
    assert n.dtype == np.float64 and np.array_equal(n, nrm.astype(np.float64))
    v, f, n = dtu_eval.read_ply(path, with_normals=True)
    assert np.array_equal(n, nrm.astype(np.float64))
    assert len(dtu_eval.read_ply(path)) == 2 and len(dtu_eval.read_ply(path, with_colors=True)) == 3
    pcd_filter.write_ply(path, xyz, rgb)
    assert dtu_eval.read_ply(path, with_colors=True, with_normals=True)[3] is None
    with open(path, "w") as fh:                                          # ASCII, as tsdf.meshwrite lays a mesh out
        fh.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
                 "property float ny\nproperty float nz\nend_header\n0 1 2 0 0 1\n3 4 5 0 1 0\n")
    v, f, n = dtu_eval.read_ply(path, with_normals=True)
    assert v.tolist() == [[0, 1, 2], [3, 4, 5]] and n.tolist() == [[0, 0, 1], [0, 1, 0]]
