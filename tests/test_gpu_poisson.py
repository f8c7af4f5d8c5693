"""Poisson surface reconstruction on the GPU (csrc/poisson.hip through uforecon_amd/ops.py and uforecon_amd/poisson_mesh.py)
against the numpy / scipy restatement poisson_ref.py on the same inputs.  The kernels sum in their own fixed order, so values
are compared within rounding bounds (stated where they are used) and two runs of the kernels are compared bit for bit."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import poisson_ref as R
from uforecon_amd import clean_mesh, dtu_eval, ops, pcd_filter, poisson_mesh
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

CENTRE = np.array([0.3, -0.2, 0.1])
TX, TY, TZ = ops.POISSON_TILE          # the nodes one block of the q = A p kernel owns at a time: 8 x 4 x 64


def _cuda(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------ splat
ORIGIN, H, DIMS = (-0.25, 0.5, 1.0), 0.5, (5, 6, 7)


def _splat_clouds():
    rng = np.random.default_rng(4)
    P, N = R.sphere_cloud(500, seed=4)
    o, h, d = R.grid(P, 8, 2)
    top = np.asarray(ORIGIN) + H * (np.asarray(DIMS) - 1)
    one = np.asarray(ORIGIN) + H * np.array([[1.3, 2.6, 3.1]])
    nodes = np.asarray(ORIGIN) + H * rng.integers(0, 5, (40, 3)).astype(np.float64)
    inside = np.asarray(ORIGIN) + H * rng.uniform(0, 4, (30, 3))
    return {"random 500 at resolution 8": (P, N, tuple(o), h, tuple(int(v) for v in d)),
            "one sample": (one, np.array([[0.0, 0.6, -0.8]]), ORIGIN, H, DIMS),
            "duplicates": (np.repeat(inside, 3, 0), rng.standard_normal((90, 3)), ORIGIN, H, DIMS),
            "on nodes": (nodes, rng.standard_normal((40, 3)), ORIGIN, H, DIMS),
            "maximum corner": (np.stack([top, top, np.asarray(ORIGIN)]), rng.standard_normal((3, 3)), ORIGIN, H, DIMS)}


@pytest.mark.parametrize("name", list(_splat_clouds()))
def test_splat_equals_the_restatement_and_repeats_its_bits(name):
    P, N, origin, h, dims = _splat_clouds()[name]
    V, W = ops.poisson_splat(_cuda(P), _cuda(N), origin, h, dims)
    assert V.shape == (3,) + tuple(dims) and W.shape == tuple(dims) and V.dtype == W.dtype == torch.float64
    Vr, Wr = R.splat(P, N, origin, h, dims)
    assert np.abs(V.cpu().numpy() - Vr).max() <= 1e-12 * np.abs(Vr).max()
    assert np.abs(W.cpu().numpy() - Wr).max() <= 1e-12 * np.abs(Wr).max()
    assert abs(float(W.sum()) - len(P)) <= 1e-12 * len(P)
    V2, W2 = ops.poisson_splat(_cuda(P), _cuda(N), origin, h, dims)
    assert _same_bits(V, V2) and _same_bits(W, W2)


def test_splat_sums_a_node_in_ascending_sample_index():
    """three samples on one node whose normals add to different fp64 values in different orders: (1e16 + 1) - 1e16 = 0, not 1"""
    p = np.asarray(ORIGIN) + H * np.array([[2.0, 2.0, 2.0]] * 3)
    n = np.array([[1e16, 0, 0], [1.0, 0, 0], [-1e16, 0, 0]])
    V, _ = ops.poisson_splat(_cuda(p), _cuda(n), ORIGIN, H, DIMS)
    assert float(V[0, 2, 2, 2]) == (1e16 + 1.0) - 1e16 == 0.0
    V, _ = ops.poisson_splat(_cuda(p[[0, 2, 1]]), _cuda(n[[0, 2, 1]]), ORIGIN, H, DIMS)
    assert float(V[0, 2, 2, 2]) == 1.0


# ------------------------------------------------------------------ divergence and one application of A
STENCIL_DIMS = [(5, 6, 7), (2, 2, 2), (65, 3, 4),
                (TX - 1, TY - 1, TZ - 1), (TX, TY, TZ), (TX + 1, TY + 1, TZ + 1), (2 * TX + 1, 2, 2 * TZ + 1)]


@pytest.mark.parametrize("dims", STENCIL_DIMS)
def test_divergence_and_laplacian_equal_the_restatement(dims):
    rng = np.random.default_rng(sum(dims))
    h = 0.37
    V = rng.standard_normal((3,) + dims)
    b = ops.poisson_divergence(_cuda(V), h).cpu().numpy()
    want = R.divergence(V, h)
    assert b.shape == dims and np.abs(b - want).max() <= 1e-12 * np.abs(want).max()
    p = rng.standard_normal(dims)
    q = ops.poisson_laplacian(_cuda(p), h).cpu().numpy()
    want = R.laplacian(p, h)
    assert q.shape == dims and np.abs(q - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ solve
@functools.lru_cache(maxsize=None)
def _system(dims):
    b = np.random.default_rng(9).standard_normal(dims)
    h = 0.07
    return b, h, (R.solve_lu(b, h) if dims == (17, 13, 11) else R.solve(b, h))      # the LU takes 6 s at 32^3 (poisson_ref.solve)


@pytest.mark.parametrize("dims", [(17, 13, 11), (32, 32, 32)])
def test_solve_equals_the_direct_solve(dims):
    b, h, want = _system(dims)
    tol = 1e-10
    x, info = ops.poisson_solve(_cuda(b), h, tol=tol, max_iter=1000)
    x = x.cpu().numpy()
    err = np.abs(x - want).max() / np.abs(want).max()
    true_res = np.linalg.norm(R.laplacian(x, h) + b) / np.linalg.norm(b)
    print("solve %s: %d iterations, residual %.3g (recurrence) %.3g (recomputed), error %.3g" %
          (dims, info["iterations"], info["residual"], true_res, err))
    assert info["converged"] and info["iterations"] % 16 == 0 and 0 < info["iterations"] < 1000
    # cond(A) <= 4 (n + 1)^2 / pi^2 = 441 at n = 32: a relative residual of 1e-10 bounds the relative error by 4.4e-8 in the
    # 2-norm; the 20x margin covers the gap to the max-norm
    assert err <= 1e-6
    assert info["residual"] <= tol and true_res <= 2 * tol


def test_solve_repeats_its_bits_and_takes_a_workspace():
    b, h, _ = _system((17, 13, 11))
    ws = torch.empty(ops.poisson_workspace_bytes(b.shape), dtype=torch.uint8, device="cuda")
    x1, i1 = ops.poisson_solve(_cuda(b), h, workspace=ws)
    x2, i2 = ops.poisson_solve(_cuda(b), h)
    assert _same_bits(x1, x2) and i1 == i2 and i1["converged"]
    with pytest.raises(UfrError, match="workspace"):
        ops.poisson_solve(_cuda(b), h, workspace=ws[:-1])


def test_solve_of_zero_is_zero_after_no_iteration():
    x, info = ops.poisson_solve(torch.zeros((9, 5, 70), dtype=torch.float64, device="cuda"), 0.1)
    assert info == dict(iterations=0, residual=0.0, converged=True)
    assert x.shape == (9, 5, 70) and not bool(x.isnan().any()) and float(x.abs().max()) == 0.0


def test_solve_reports_max_iter_instead_of_raising():
    b, h, _ = _system((32, 32, 32))
    x, info = ops.poisson_solve(_cuda(b), h, tol=1e-10, max_iter=3)
    assert info["iterations"] == 3 and info["converged"] is False and 0.0 < info["residual"] < 1.0
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0.0


def test_solve_of_a_tiny_grid_survives_an_exact_zero_residual():
    """(2,2,2) has four distinct eigenvalues: conjugate gradients end long before the first look; alpha and beta then are
    quotients of values at rounding level or 0, which must not become NaN"""
    b = np.random.default_rng(5).standard_normal((2, 2, 2))
    x, info = ops.poisson_solve(_cuda(b), 1.0, tol=1e-12)
    assert info["converged"] and bool(torch.isfinite(x).all())
    # |e|_2 <= tol |b|_2 / lambda_min with lambda_min = 3 (2 - 2 cos(pi / 3)) = 3 and |b|_2 <= sqrt(8) max |b|: 0.94e-12 max |b|;
    # ten times that for the distance between the recurrence's residual and the true one
    assert np.abs(x.cpu().numpy() - R.solve_lu(b, 1.0)).max() <= 1e-11 * np.abs(b).max()


# ------------------------------------------------------------------ the spheres, end to end
@functools.lru_cache(maxsize=None)
def _full_sphere():
    P, N = R.sphere_cloud()
    return P, N, poisson_mesh.reconstruct(P, N, resolution=32, pad=3)


def test_full_sphere_is_a_closed_outward_surface_within_half_a_cell():
    P, N, (verts, faces, normals, density, colors, info) = _full_sphere()
    assert info["dims"] == [39, 39, 39] and info["converged"] and info["dropped"] == 0 and colors is None
    v, f = verts.cpu().numpy(), faces.cpu().numpy().astype(np.int64)
    d = np.abs(np.linalg.norm(v - CENTRE, axis=1) - 1.0) / info["h"]
    print("full sphere on the GPU: worst vertex %.4f h, %d vertices, %d iterations" % (d.max(), len(v), info["iterations"]))
    assert len(v) > 1000 and d.max() <= 0.5
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all()                                           # every edge lies in exactly two faces
    assert len(v) - len(counts) + len(f) == 2                            # Euler characteristic of a sphere
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3.0 - CENTRE) > 0.0).all()
    assert (np.einsum("ij,ij->i", normals.cpu().numpy().astype(np.float64), v - CENTRE) > 0.0).all()
    assert float(density.min()) >= 0.0 and float(density.max()) > 1.0


def test_full_sphere_repeats_its_bits():
    P, N, first = _full_sphere()
    again = poisson_mesh.reconstruct(P, N, resolution=32, pad=3)
    for a, b in zip(first[:4], again[:4]):
        assert _same_bits(a, b)
    assert first[5] == again[5]


def test_iso_and_density_equal_the_restatement():
    P, N, (verts, _, _, density, _, info) = _full_sphere()
    origin, h, dims = R.grid(P, 32, 3)
    assert info["h"] == h and info["origin"] == origin.tolist() and info["dims"] == dims.tolist()
    V, W = R.splat(P, N, origin, h, dims)
    chi = R.solve(R.divergence(V, h), h)                  # the restatement's field through the kernel's sampler: rounding only
    values, mean = ops.poisson_sample(_cuda(chi), origin, h, _cuda(P), return_mean=True)
    assert np.abs(values.cpu().numpy() - R.sample(chi, origin, h, P)).max() <= 1e-12 * np.abs(chi).max()
    assert abs(float(mean) - R.iso_value(chi, origin, h, P)) <= 1e-12 * np.abs(chi).max()
    # the kernel's own field stops at tol = 1e-6: |e|_2 <= cond(A) tol |chi|_2 with cond(A) <= 4 (n + 1)^2 / pi^2, and iso is
    # an average of interpolated values, so it moves by at most max |e| <= |e|_2
    assert abs(info["iso"] - float(mean)) <= 4 * 40 ** 2 / np.pi ** 2 * 1e-6 * np.linalg.norm(chi)
    want = R.sample(W, origin, h, verts.cpu().numpy())
    assert np.abs(density.cpu().numpy() - want).max() <= 1e-12 * want.max()


@functools.lru_cache(maxsize=None)
def _partial_sphere():
    P, N = R.sphere_cloud(20000, z_min=-0.3)
    return P, N, poisson_mesh.reconstruct(P, N, resolution=32, pad=4), poisson_mesh.reconstruct(P, N, resolution=32, pad=4, min_density=0.25)


def test_partial_sphere_trim_keeps_the_cap_and_removes_the_closure():
    P, N, full, cut = _partial_sphere()
    assert len(P) == 12932
    h = full[5]["h"]
    va, fa, vk, fk = full[0].cpu().numpy(), full[1].cpu().numpy(), cut[0].cpu().numpy(), cut[1].cpu().numpy()
    kept = np.abs(np.linalg.norm(vk - CENTRE, axis=1) - 1.0) / h
    every = np.abs(np.linalg.norm(va - CENTRE, axis=1) - 1.0) / h
    keep = full[3].cpu().numpy() >= 0.25
    above = va[:, 2] - CENTRE[2] > -0.15
    print("partial sphere on the GPU: worst kept vertex %.4f h, worst untrimmed %.2f h, lost above -0.15: %d of %d" %
          (kept.max(), every.max(), int((above & ~keep).sum()), int(above.sum())))
    assert kept.max() <= 1.5                         # the restatement measures 1.0521 h, at the rim (tests/test_poisson_ref.py)
    assert above.sum() > 1000 and not (above & ~keep).any()
    assert every.max() > 5.0                         # the closure far from the samples: the trim is not vacuous
    # compact indices, order preserved, only kept vertices
    assert np.array_equal(vk, va[keep]) and np.array_equal(cut[3].cpu().numpy(), full[3].cpu().numpy()[keep])
    assert np.array_equal(cut[2].cpu().numpy(), full[2].cpu().numpy()[keep])
    vr, fr, _ = R.trim(va, fa, full[3].cpu().numpy(), 0.25)
    assert np.array_equal(fk, fr) and fk.dtype == np.int32 and fk.min() >= 0 and fk.max() < len(vk) and 0 < len(fk) < len(fa)


# ------------------------------------------------------------------ colours
def test_vertex_colours_are_the_nearest_samples_with_ties_to_the_lowest_index():
    P, N = R.sphere_cloud(600, seed=8)
    rng = np.random.default_rng(8)
    P, N = np.concatenate([P, P[:200]]), np.concatenate([N, N[:200]])         # 200 exact duplicates: every vertex near one has a tie
    col = rng.integers(0, 256, (800, 3)).astype(np.uint8)
    col[600:] = 255 - col[:200]
    verts, _, _, _, vcol, _ = poisson_mesh.reconstruct(P, N, col, resolution=16, pad=3)
    v = verts.cpu().numpy()
    want = R.nearest_colours(v, P, col)
    assert vcol.dtype == torch.uint8 and np.array_equal(vcol.cpu().numpy(), want)
    nearest = np.array([np.argmin(((P - x) ** 2).sum(1)) for x in v])
    assert (nearest < 200).sum() > 20                                           # the tie was met, and the first of the pair won


# ------------------------------------------------------------------ argument errors
def test_argument_errors_are_ufr_errors():
    P, N = R.sphere_cloud(100, seed=1)
    for kw in (dict(resolution=3), dict(pad=1), dict(resolution=1400)):
        with pytest.raises(UfrError):
            poisson_mesh.reconstruct(P, N, **kw)
    with pytest.raises(UfrError, match="degenerate"):
        poisson_mesh.reconstruct(np.ones((10, 3)), N[:10])
    bad = P.copy()
    bad[3, 1] = np.inf
    with pytest.raises(UfrError, match="NaN or infinite"):
        poisson_mesh.reconstruct(bad, N)
    with pytest.raises(UfrError, match="normal"):
        poisson_mesh.reconstruct(P, np.zeros_like(N))
    with pytest.raises(UfrError):
        ops.poisson_laplacian(torch.zeros((4, 1, 4), dtype=torch.float64, device="cuda"), 1.0)
    with pytest.raises(UfrError):
        ops.poisson_solve(torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda"), 1.0)
    with pytest.raises(UfrError):
        ops.poisson_solve(torch.full((4, 4, 4), float("nan"), dtype=torch.float64, device="cuda"), 1.0)
    Nz = N.copy()
    Nz[:5] = 0.0
    Nz[5, 0] = np.nan
    assert poisson_mesh.reconstruct(P, Nz, resolution=8)[5]["dropped"] == 6


# ------------------------------------------------------------------ the command
def _write_cameras(root, centres):
    os.makedirs(os.path.join(root, "cameras"))
    for v, c in enumerate(centres):
        E = np.eye(4)
        E[:3, 3] = -np.asarray(c)
        with open(os.path.join(root, "cameras", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(str(x) for x in row) for row in E) + "\n\nintrinsic\n1 0 0\n0 1 0\n0 0 1\n\n425 2.5\n")


def test_command_writes_meshes_that_the_other_commands_read(tmp_path, capsys):
    P, N = R.sphere_cloud(3000, seed=2)
    rgb = np.random.default_rng(2).integers(0, 256, (len(P), 3)).astype(np.uint8)
    os.makedirs(tmp_path / "in" / "pcd")
    src = str(tmp_path / "in" / "pcd" / "scan1.ply")
    pcd_filter.write_ply(src, P.astype(np.float32), rgb, N.astype(np.float32))
    out = tmp_path / "out"
    assert poisson_mesh.main(["--root_dir", str(tmp_path / "in"), "--out_dir", str(out), "--resolution", "24", "--pad", "3", "--color"]) == 0
    assert "scan1" in capsys.readouterr().out
    mesh = str(out / "mesh" / "scan1.ply")
    v, f = clean_mesh.read_ply(mesh)
    v2, f2, c2, n2 = dtu_eval.read_ply(mesh, with_colors=True, with_normals=True)
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and f.dtype == np.int32 and c2.shape == v.shape and n2.shape == v.shape
    assert len(v) > 500 and f.max() == len(v) - 1
    assert np.abs(np.linalg.norm(v - CENTRE, axis=1) - 1.0).max() <= 0.5 * 2.0 / 24 + 1e-5        # half a cell, + the %f of the file
    report = json.load(open(out / "poisson_mesh.json"))
    info = report["scans"]["scan1"]
    assert set(info) >= {"dims", "h", "origin", "iso", "iterations", "residual", "converged", "dropped", "vertices", "faces"}
    assert info["converged"] and info["vertices"] == len(v) and info["faces"] == len(f) and report["params"]["resolution"] == 24
    # the same cloud without normals: one line, a non-zero status, no report
    bare = str(tmp_path / "in" / "pcd" / "scan2.ply")
    pcd_filter.write_ply(bare, P.astype(np.float32), rgb)
    out2 = tmp_path / "out2"
    assert poisson_mesh.main(["--root_dir", str(tmp_path / "in"), "--out_dir", str(out2), "--scans", "2"]) != 0
    said = capsys.readouterr().out.strip().splitlines()
    assert len(said) == 1 and "no normals" in said[0] and not os.path.exists(out2 / "poisson_mesh.json")
    # ... and with --normals 16 and viewpoints around the sphere
    _write_cameras(str(tmp_path / "data"), [CENTRE + 6.0 * np.array(a) for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))])
    assert poisson_mesh.main(["--root_dir", str(tmp_path / "in"), "--out_dir", str(out2), "--scans", "2", "--resolution", "24", "--pad", "3",
                              "--normals", "16", "--dataset_dir", str(tmp_path / "data"), "--views", "0", "1", "2", "3", "4", "5"]) == 0
    v3, f3 = dtu_eval.read_ply(str(out2 / "mesh" / "scan2.ply"))
    assert len(f3) > 500 and np.abs(np.linalg.norm(v3 - CENTRE, axis=1) - 1.0).max() <= 2.0 / 24
    assert json.load(open(out2 / "poisson_mesh.json"))["scans"]["scan2"]["converged"]
