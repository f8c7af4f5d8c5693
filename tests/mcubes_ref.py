"""numpy restatement of the marching-cubes kernel of csrc/mcubes.hip (include/ufr.h, ufr_marching_cubes_*): the same
semantics in fp32, vectorised, so that the kernel's verts / faces can be compared bit for bit.

``table`` is the kernel's own case table ((256, 16) int8, ufr_marching_cubes_table): triangles as edge triples, -1
padded.  Edge e = 4 * axis + r joins corner c and c + (1 << axis) of the cube, c = dx | dy << 1 | dz << 2 with bit axis
clear and the other two bits, the lower axis first, = r & 1, r >> 1.
"""
from __future__ import annotations

import numpy as np


def edge_owner_offsets():
    """(12, 3) corner offset of each edge's lower end, (12,) its axis."""
    off = np.zeros((12, 3), np.int64)
    axis = np.zeros(12, np.int64)
    for e in range(12):
        a, r = e // 4, e % 4
        others = [b for b in range(3) if b != a]
        off[e, others[0]] = r & 1
        off[e, others[1]] = r >> 1
        axis[e] = a
    return off, axis


def crossing_mask(vol, level=0.0):
    """(X,Y,Z) uint8: bit a set iff the edge from voxel p to p + e_a exists and exactly one end is below the level."""
    below = vol < np.float32(level)
    mask = np.zeros(vol.shape, np.uint8)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a] = slice(0, -1)
        hi[a] = slice(1, None)
        mask[tuple(lo)] |= ((below[tuple(lo)] != below[tuple(hi)]).astype(np.uint8) << a)
    return mask


def _gradient(vol, a):
    """(X,Y,Z) fp32 derivative along axis a: (f[i+1] - f[i-1]) * 0.5 inside, one-sided differences at the border."""
    f = np.moveaxis(vol, a, 0)
    g = np.empty_like(f)
    g[1:-1] = (f[2:] - f[:-2]) * np.float32(0.5)
    g[0] = f[1] - f[0]
    g[-1] = f[-1] - f[-2]
    return np.moveaxis(g, 0, a)


def vertices(vol, level=0.0):
    """verts (V,3) fp32, normals (V,3) fp32 in (owner voxel, axis) order; mask; first vertex id per voxel (-1: none)."""
    vol = np.ascontiguousarray(vol, np.float32)
    lv = np.float32(level)
    mask = crossing_mask(vol, level)
    bits = ((mask[..., None] >> np.arange(3, dtype=np.uint8)) & 1).astype(bool).reshape(-1, 3)   # (N, 3)
    vox, axis = np.nonzero(bits)                      # row-major: voxel linear index, then axis
    X, Y, Z = vol.shape
    p = np.stack(np.unravel_index(vox, vol.shape), axis=1)        # (V, 3)
    q = p.copy()
    q[np.arange(len(q)), axis] += 1
    flat = vol.reshape(-1)
    a = flat[vox]
    b = vol[q[:, 0], q[:, 1], q[:, 2]]
    t = (lv - a) / (b - a)
    verts = p.astype(np.float32)
    verts[np.arange(len(verts)), axis] = verts[np.arange(len(verts)), axis] + t
    grads = [_gradient(vol, d) for d in range(3)]
    n = np.empty((len(vox), 3), np.float32)
    for d in range(3):
        g0 = grads[d][p[:, 0], p[:, 1], p[:, 2]]
        g1 = grads[d][q[:, 0], q[:, 1], q[:, 2]]
        n[:, d] = g0 + t * (g1 - g0)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = ln > 0
    normals = np.zeros_like(n)
    normals[ok] = n[ok] / ln[ok, None]
    counts = bits.sum(1)
    first = np.full(vol.size, -1, np.int64)
    has = counts > 0
    first[has] = (np.cumsum(counts) - counts)[has]
    return verts, normals, mask, first.reshape(vol.shape)


def cube_cases(vol, level=0.0):
    """(X-1,Y-1,Z-1) case index of every cube (bit c set iff corner c = dx | dy << 1 | dz << 2 is below)."""
    below = (np.asarray(vol) < np.float32(level)).astype(np.int64)
    case = np.zeros(tuple(s - 1 for s in below.shape), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= below[dx:dx + case.shape[0], dy:dy + case.shape[1], dz:dz + case.shape[2]] << c
    return case


def marching_cubes(vol, table, level=0.0):
    """(verts (V,3) fp32, faces (F,3) int32, normals (V,3) fp32) as csrc/mcubes.hip computes them."""
    vol = np.ascontiguousarray(vol, np.float32)
    table = np.asarray(table, np.int64).reshape(256, -1)
    verts, normals, mask, first = vertices(vol, level)
    case = cube_cases(vol, level)
    ntri = (table >= 0).sum(1) // 3
    X, Y, Z = vol.shape
    cx, cy, cz = np.nonzero(ntri[case] > 0)           # cube origins in linear order
    cs = case[cx, cy, cz]
    k = ntri[cs]
    rep = np.repeat(np.arange(len(cs)), k)
    slot = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)   # triangle number within its cube
    off, eaxis = edge_owner_offsets()
    faces = np.empty((len(rep), 3), np.int64)
    for j in range(3):
        e = table[cs[rep], 3 * slot + j]
        ox, oy, oz = cx[rep] + off[e, 0], cy[rep] + off[e, 1], cz[rep] + off[e, 2]
        ax = eaxis[e]
        below_bits = mask[ox, oy, oz].astype(np.int64) & ((1 << ax) - 1)
        pc = (below_bits & 1) + ((below_bits >> 1) & 1)
        faces[:, j] = first[ox, oy, oz] + pc
    return verts, faces.astype(np.int32), normals
