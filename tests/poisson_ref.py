"""numpy / scipy restatement of the uniform-grid Poisson reconstruction of csrc/poisson.hip and uforecon_amd/poisson_mesh.py
(include/ufr.h, "Poisson surface reconstruction"): the grid, the trilinear splat, the divergence, the matrix A as a scipy
sparse matrix with a direct solve, the iso value, the densities, the trim and the colour transfer.  No GPU.  Sums that the
kernels take in a fixed order are taken here in numpy's order: results agree to rounding, not bit for bit."""
from __future__ import annotations

import numpy as np


def sphere_cloud(n=4000, seed=0, radius=1.0, centre=(0.3, -0.2, 0.1), z_min=None):
    """``n`` unit vectors of default_rng(seed) as normals, the points at centre + radius * normal; ``z_min``: only the draws
    with normal z > z_min are kept (a partial sphere)."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    nrm = v / np.linalg.norm(v, axis=1, keepdims=True)
    if z_min is not None:
        nrm = nrm[nrm[:, 2] > z_min]
    return np.asarray(centre, np.float64) + radius * nrm, nrm


def keep_mask(normals):
    """samples whose normal is finite and not 0"""
    normals = np.asarray(normals, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(normals).all(1) & ((normals * normals).sum(1) > 0.0)


def grid(points, resolution=256, pad=4):
    """(origin (3,), h, dims (3,) int) -- ValueError for what ufr_poisson_grid refuses"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    if resolution < 4 or pad < 2:
        raise ValueError("resolution < 4 or pad < 2")
    if len(points) == 0 or not np.isfinite(points).all():
        raise ValueError("empty cloud or coordinates that are not finite")
    mn, mx = points.min(0), points.max(0)
    h = (mx - mn).max() / float(resolution)
    if not (h > 0.0 and np.isfinite(h) and h * h > 0.0 and np.isfinite(1.0 / (h * h))):
        raise ValueError("degenerate extent")
    dims = np.ceil((mx - mn) / h).astype(np.int64) + 1 + 2 * pad
    if int(dims[0]) * int(dims[1]) * int(dims[2]) >= 2 ** 31:
        raise ValueError("2^31 nodes or more")
    return mn - pad * h, float(h), dims


def cells(points, origin, h, dims):
    """(cell (N,3) int64, t (N,3)): u = (p - origin) / h clamped to [0, dim - 1]; cell = min(floor(u), dim - 2); t = u - cell"""
    dims = np.asarray(dims, np.int64)
    u = (np.asarray(points, np.float64) - np.asarray(origin, np.float64)) / h
    u = np.minimum(np.maximum(u, 0.0), (dims - 1).astype(np.float64))
    c = np.minimum(np.floor(u).astype(np.int64), dims - 2)
    return c, u - c


def corner_weights(t):
    """(N,8): corner 4a + 2b + g has the weight (wx * wy) * wz"""
    w = np.empty((len(t), 8))
    for corner in range(8):
        a, b, g = (corner >> 2) & 1, (corner >> 1) & 1, corner & 1
        wx = t[:, 0] if a else 1.0 - t[:, 0]
        wy = t[:, 1] if b else 1.0 - t[:, 1]
        wz = t[:, 2] if g else 1.0 - t[:, 2]
        w[:, corner] = (wx * wy) * wz
    return w


def corner_nodes(c, dims):
    """(N,8) linear node index of every corner"""
    out = np.empty((len(c), 8), np.int64)
    for corner in range(8):
        a, b, g = (corner >> 2) & 1, (corner >> 1) & 1, corner & 1
        out[:, corner] = ((c[:, 0] + a) * dims[1] + (c[:, 1] + b)) * dims[2] + (c[:, 2] + g)
    return out


def splat(points, normals, origin, h, dims):
    """V (3,X,Y,Z), W (X,Y,Z)"""
    dims = tuple(int(d) for d in dims)
    c, t = cells(points, origin, h, dims)
    w, node = corner_weights(t), corner_nodes(c, dims)
    nn = dims[0] * dims[1] * dims[2]
    V = np.zeros((3, nn))
    W = np.zeros(nn)
    np.add.at(W, node.reshape(-1), w.reshape(-1))
    for a in range(3):
        np.add.at(V[a], node.reshape(-1), (w * np.asarray(normals, np.float64)[:, a:a + 1]).reshape(-1))
    return V.reshape((3,) + dims), W.reshape(dims)


def divergence(V, h):
    """b = ((dx + dy) + dz) / (2h) by central differences, V = 0 outside"""
    d = []
    for a in range(3):
        f = np.pad(V[a], [(1, 1) if b == a else (0, 0) for b in range(3)])
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[a], lo[a] = slice(2, None), slice(0, -2)
        d.append(f[tuple(hi)] - f[tuple(lo)])
    return ((d[0] + d[1]) + d[2]) / (2.0 * h)


def laplacian(p, h):
    """A p: (6 p - the six neighbours) / h^2, p = 0 outside"""
    f = np.pad(p, 1)
    s = ((f[:-2, 1:-1, 1:-1] + f[2:, 1:-1, 1:-1]) + (f[1:-1, :-2, 1:-1] + f[1:-1, 2:, 1:-1])) + (f[1:-1, 1:-1, :-2] + f[1:-1, 1:-1, 2:])
    return (6.0 * p - s) / (h * h)


def matrix(dims, h):
    """A as a scipy CSR matrix over the z-fastest node order"""
    import scipy.sparse as sp

    def second(n):
        return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])

    X, Y, Z = (int(d) for d in dims)
    eye = sp.identity
    A = sp.kron(sp.kron(second(X), eye(Y)), eye(Z)) + sp.kron(sp.kron(eye(X), second(Y)), eye(Z)) + sp.kron(sp.kron(eye(X), eye(Y)), second(Z))
    return (A / (h * h)).tocsr()


def solve_lu(b, h):
    """chi with A chi = -b, by scipy's sparse LU of ``matrix``.  Its fill-in grows fast in 3-D (6 s at 32^3, half a minute at
    39^3): for small grids."""
    from scipy.sparse.linalg import splu

    return splu(matrix(b.shape, h).tocsc()).solve(-b.reshape(-1)).reshape(b.shape)


def solve(b, h):
    """chi with A chi = -b, directly, by fast diagonalisation: A is the Kronecker sum of three 1-D second-difference matrices
    with zero walls, whose eigenvectors are the sines of scipy.fft's DST-I and whose eigenvalues are (2 - 2 cos(pi m / (n +
    1))) / h^2, m = 1 .. n.  Milliseconds at any test size; tests/test_poisson_ref.py checks it against ``solve_lu`` and
    against ``matrix`` itself (the residual of A chi + b)."""
    from scipy.fft import dstn, idstn

    lam = [2.0 - 2.0 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1)) for n in b.shape]
    L = ((lam[0][:, None, None] + lam[1][None, :, None]) + lam[2][None, None, :]) / (h * h)
    return idstn(dstn(-np.asarray(b, np.float64), type=1) / L, type=1)


def sample(vol, origin, h, points):
    """the trilinear value of vol at every point"""
    c, t = cells(points, origin, h, vol.shape)
    return (corner_weights(t) * vol.reshape(-1)[corner_nodes(c, vol.shape)]).sum(1)


def iso_value(chi, origin, h, points):
    return float(sample(chi, origin, h, points).mean())


def trim(verts, faces, density, min_density):
    """(verts, faces, kept vertex mask): vertices below the threshold and every face that touches one are dropped; indices
    are compacted and the order is kept"""
    keep = np.asarray(density) >= min_density
    fkeep = keep[faces].all(1) if len(faces) else np.zeros(0, bool)
    remap = np.cumsum(keep) - 1
    return verts[keep], remap[faces[fkeep]].astype(np.int32), keep


def nearest_colours(verts, points, colours):
    """the colour of every vertex's nearest sample, ties to the lowest index (brute force)"""
    out = np.empty((len(verts), 3), np.uint8)
    for i, v in enumerate(np.asarray(verts, np.float64)):
        d = points - v
        out[i] = colours[np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])]
    return out


def reconstruct(points, normals, table, resolution=256, pad=4, min_density=0.0):
    """The whole chain on the host, the mesh by tests/mcubes_ref.py (``table``: ops.marching_cubes_table()).  Returns
    dict(verts (scene coordinates, fp64), faces, normals, density, keep (mask over the untrimmed vertices), verts_all,
    origin, h, dims, iso, chi, dropped)."""
    import mcubes_ref

    points, normals = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    ok = keep_mask(normals)
    points, normals = points[ok], normals[ok]
    origin, h, dims = grid(points, resolution, pad)
    V, W = splat(points, normals, origin, h, dims)
    chi = solve(divergence(V, h), h)
    iso = iso_value(chi, origin, h, points)
    v, f, n = mcubes_ref.marching_cubes((chi - iso).astype(np.float32), table, 0.0)
    verts_all = origin + h * v.astype(np.float64)
    density = sample(W, origin, h, verts_all)
    verts, faces, keep = trim(verts_all, f, density, min_density)
    return dict(verts=verts, faces=faces, normals=n[keep], density=density[keep], keep=keep, verts_all=verts_all, origin=origin, h=h,
                dims=dims, iso=iso, chi=chi, dropped=int((~ok).sum()))
