"""numpy float64 restatement of mesh texturing (include/ufr.h, "mesh texturing"; csrc/mesh_texture.hip and the textured branch
of csrc/raster.hip's shade kernel): the closed-form atlas, the bake of one texel from the photographs, the Jacobi round of the
texel-space fill and the textured shade, with the kernels' expressions and summation orders.  The per-view rule is
color_mesh_ref.vertex_color, the ray generator, first hit and shading are raster_ref's, both imported as they are.  Python
floats are IEEE doubles and every product below is a statement of its own, so nothing is fused.  Texel by texel, slow and plain
on purpose.
"""
import math

import numpy as np

import color_mesh_ref as CR
import raster_ref as RR

MAX_PATCH, MAX_SIDE = 125, 16384


# ------------------------------------------------------------------ the atlas
def layout(F, S):
    """(Ht, Wt, cols, rows): cells of side S + 3, two faces a cell, cols = ceil(sqrt(cells)) in integers"""
    assert 1 <= S <= MAX_PATCH and F >= 1
    cells = (F + 1) // 2
    cols = 1
    while cols * cols < cells:
        cols += 1
    rows = -(-cells // cols)
    C = S + 3
    assert cols * C <= MAX_SIDE and rows * C <= MAX_SIDE
    return rows * C, cols * C, cols, rows


def owner(F, S, x, y):
    """(face, i, j) of texel (x, y): the face it belongs to (-1: none) and its place in that face's patch"""
    _, _, cols, _ = layout(F, S)
    C = S + 3
    cx, cy = x // C, y // C
    i, j = x - cx * C, y - cy * C
    f = 2 * (cy * cols + cx)
    if i + j > S + 2:
        f, i, j = f + 1, C - 1 - i, C - 1 - j
    return (f if f < F else -1), i, j


def owner_map(F, S):
    """(face, i, j) as (Ht,Wt) int64 arrays, by ``owner`` texel by texel"""
    Ht, Wt, _, _ = layout(F, S)
    out = np.zeros((3, Ht, Wt), np.int64)
    for y in range(Ht):
        for x in range(Wt):
            out[:, y, x] = owner(F, S, x, y)
    return out[0], out[1], out[2]


def corner_texels(F, S):
    """(F,3,2) float64: texel (x, y) of corners a, b, c -- local (0,0), (S,0), (0,S) for the even face of a cell, the half turn
    (C-1,C-1), (C-1-S,C-1), (C-1,C-1-S) for the odd one"""
    _, _, cols, _ = layout(F, S)
    C = S + 3
    out = np.zeros((F, 3, 2))
    for f in range(F):
        q = f // 2
        ox, oy = (q % cols) * C, (q // cols) * C
        loc = [(0, 0), (S, 0), (0, S)]
        if f % 2:
            loc = [(C - 1 - i, C - 1 - j) for i, j in loc]
        out[f] = [(ox + i, oy + j) for i, j in loc]
    return out


def weights(i, j, S):
    wb, wc = float(i) / float(S), float(j) / float(S)
    return (1.0 - wb) - wc, wb, wc


def footprint(tx, ty):
    """[(x, y, weight)] of the four texels under the bilinear footprint of texel-space point (tx, ty), unclamped"""
    x0, y0 = math.floor(tx), math.floor(ty)
    fx, fy = tx - x0, ty - y0
    return [(x0, y0, (1 - fx) * (1 - fy)), (x0 + 1, y0, fx * (1 - fy)), (x0, y0 + 1, (1 - fx) * fy), (x0 + 1, y0 + 1, fx * fy)]


# ------------------------------------------------------------------ the bake
def face_normal(a, b, c):
    """(b - a) x (c - a) / its length, each component two products and a difference; zero when the length is not > 0 or not
    finite"""
    with np.errstate(all="ignore"):
        u = [np.float64(b[k]) - np.float64(a[k]) for k in range(3)]
        w = [np.float64(c[k]) - np.float64(a[k]) for k in range(3)]
        n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if not (ln > 0 and np.isfinite(ln)):
            return [0.0, 0.0, 0.0]
        return [float(n[k] / ln) for k in range(3)]


def bake(verts, faces, images, depth, k, w2c, centre, S, fallback=None, fill=(128, 128, 128), **kw):
    """texture (Ht,Wt,3) uint8 and views_used (Ht,Wt) uint8 of the atlas of ``layout(F, S)``; ``kw``: z_min, depth_tol, min_cos,
    power, mode of ``color_mesh_ref.vertex_color``"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    images = np.asarray(images, np.uint8)
    depth = None if depth is None else np.asarray(depth, np.float32)
    k, w2c, centre = np.asarray(k, np.float64), np.asarray(w2c, np.float64), np.asarray(centre, np.float64)
    V, F = len(verts), len(faces)
    Ht, Wt, _, _ = layout(F, S)
    texture = np.zeros((Ht, Wt, 3), np.uint8)
    used = np.zeros((Ht, Wt), np.uint8)
    texture[:] = np.asarray(fill, np.uint8)
    normals = {}
    for y in range(Ht):
        for x in range(Wt):
            f, i, j = owner(F, S, x, y)
            if f < 0:
                continue
            ia, ib, ic = (int(t) for t in faces[f])
            if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= V:
                continue
            a, b, c = verts[ia], verts[ib], verts[ic]
            if f not in normals:
                normals[f] = face_normal(a, b, c)
            wa, wb, wc = weights(i, j, S)
            with np.errstate(all="ignore"):
                p = [float((np.float64(wa) * a[t] + np.float64(wb) * b[t]) + np.float64(wc) * c[t]) for t in range(3)]
            col, n_used = CR.vertex_color(p, normals[f], images, depth, k, w2c, centre, fill=fill, **kw)
            if n_used == 0 and fallback is not None:
                Ca, Cb, Cc = (np.asarray(fallback[t], np.float64) for t in (ia, ib, ic))
                col = tuple(CR._to_byte(float((wa * Ca[t] + wb * Cb[t]) + wc * Cc[t])) for t in range(3))
            texture[y, x], used[y, x] = col, n_used
    return texture, used


# ------------------------------------------------------------------ the fill
def fill_round(texture, state, F, S):
    """One Jacobi round: (texture, state, filled).  An empty texel of a face visits (x-1,y), (x+1,y), (x,y-1), (x,y+1); a
    neighbour counts when it is inside the atlas, of the same face and has a state; integer mean, half to even."""
    texture, state = np.asarray(texture, np.uint8), np.asarray(state, np.uint8)
    Ht, Wt = state.shape
    assert (Ht, Wt) == layout(F, S)[:2]
    out_t, out_s, filled = texture.copy(), state.copy(), 0
    for y in range(Ht):
        for x in range(Wt):
            f = owner(F, S, x, y)[0]
            if state[y, x] != 0 or f < 0:
                continue
            tot, count = [0, 0, 0], 0
            for ux, uy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if not (0 <= ux < Wt and 0 <= uy < Ht) or owner(F, S, ux, uy)[0] != f or state[uy, ux] == 0:
                    continue
                for ch in range(3):
                    tot[ch] += int(texture[uy, ux, ch])
                count += 1
            if count > 0:
                out_t[y, x] = [CR._mean_half_even(t, count) for t in tot]
                out_s[y, x] = 1
                filled += 1
    return out_t, out_s, filled


def fill(texture, views_used, F, S, rounds):
    """Up to ``rounds`` rounds, ending after a round that fills nothing (which is counted): (texture, state, rounds_run)"""
    texture = np.asarray(texture, np.uint8).copy()
    state = (np.asarray(views_used) != 0).astype(np.uint8)
    run = 0
    while run < rounds:
        texture, state, filled = fill_round(texture, state, F, S)
        run += 1
        if filled == 0:
            break
    return texture, state, run


# ------------------------------------------------------------------ the textured shade
def render(verts, faces, k_inv, c2w, H, W, corner_xy, texture, normals=None, ambient=0.25, background=(255, 255, 255), hit=None):
    """One frame as raster_ref.render gives it, with the colour taken from ``texture`` (Ht,Wt,3) uint8 at the barycentric mix
    of the face's corner texels ``corner_xy`` (F,3,2): tx = (w_a xa + w_b xb) + w_c xc, bilinear with the indices clamped to the
    texture after the fractions are formed, colour = s / 255; a coordinate that is not finite gives white.  depth, face_id,
    normal and the first-hit part of ``close`` are raster_ref's own; ``close`` also marks a pixel whose 255 * colour * I lies
    within HALF_MARGIN of a half-integer."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    corner_xy = np.asarray(corner_xy, np.float64)
    T = np.asarray(texture, np.uint8).astype(np.float64)
    Ht, Wt = T.shape[:2]
    out = RR.render(verts, faces, k_inv, c2w, H, W, normals=normals, ambient=ambient, background=background, hit=hit)
    face_id = out["face_id"]
    on = face_id >= 0
    if not on.any():
        return out
    o, d32 = RR.rays(k_inv, c2w, H, W)
    o = o.astype(np.float64)
    d = d32[on].astype(np.float64)
    fid = face_id[on]
    fc = faces[fid]
    a, b, c = verts[fc[:, 0]] - o, verts[fc[:, 1]] - o, verts[fc[:, 2]] - o
    e0 = RR._dot(d, RR._cross_ordered(b, fc[:, 1], c, fc[:, 2]))
    e1 = RR._dot(d, RR._cross_ordered(c, fc[:, 2], a, fc[:, 0]))
    e2 = RR._dot(d, RR._cross_ordered(a, fc[:, 0], b, fc[:, 1]))
    s = (e0 + e1) + e2
    w0, w1, w2 = e0 / s, e1 / s, e2 / s
    n = RR._cross(b - a, c - a)
    N = n / np.sqrt(RR._dot(n, n))[:, None]
    if normals is not None:
        nm = np.asarray(normals, np.float64)
        Ns = (w0[:, None] * nm[fc[:, 0]] + w1[:, None] * nm[fc[:, 1]]) + w2[:, None] * nm[fc[:, 2]]
        ln = np.sqrt(RR._dot(Ns, Ns))
        with np.errstate(all="ignore"):
            N = np.where((ln > 0)[:, None], Ns / ln[:, None], N)
    I = ambient + (1.0 - ambient) * np.abs(RR._dot(N, d))
    xy = corner_xy[fid]
    with np.errstate(all="ignore"):
        tx = (w0 * xy[:, 0, 0] + w1 * xy[:, 1, 0]) + w2 * xy[:, 2, 0]
        ty = (w0 * xy[:, 0, 1] + w1 * xy[:, 1, 1]) + w2 * xy[:, 2, 1]
    ok = np.isfinite(tx) & np.isfinite(ty)
    txs, tys = np.where(ok, tx, 0.0), np.where(ok, ty, 0.0)
    x0, y0 = np.floor(txs), np.floor(tys)
    fx, fy = txs - x0, tys - y0
    xa, xb = np.clip(x0, 0, Wt - 1).astype(np.int64), np.clip(x0 + 1, 0, Wt - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, Ht - 1).astype(np.int64), np.clip(y0 + 1, 0, Ht - 1).astype(np.int64)
    gx, gy = (1.0 - fx)[:, None], (1.0 - fy)[:, None]
    fx, fy = fx[:, None], fy[:, None]
    smp = gy * (gx * T[ya, xa] + fx * T[ya, xb]) + fy * (gx * T[yb, xa] + fx * T[yb, xb])
    col = np.where(ok[:, None], smp / 255.0, 1.0)
    val = (255.0 * col) * I[:, None]
    image = out["image"].copy()
    image[on] = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    close = out["close"].copy()
    close[on] |= (np.abs(np.abs(val - np.floor(val)) - 0.5) < RR.HALF_MARGIN).any(1)
    out["image"], out["close"] = image, close
    return out
