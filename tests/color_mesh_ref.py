"""numpy float64 restatement of mesh colouring (include/ufr.h, "mesh colouring"; csrc/mesh_color.hip): the colour of one
vertex from the photographs, view by view, and the Jacobi round of the neighbour fill, with the kernels' expressions and
summation orders.  Python floats are IEEE doubles and every product below is a statement of its own, so nothing is fused.
Vertex by vertex, slow and plain on purpose.
"""
import math
import os

import numpy as np

MODE_MEAN, MODE_BEST = "mean", "best"


def _finite(*v):
    return all(math.isfinite(x) for x in v)


def _to_byte(v):
    """rint (half to even) clamped to 0..255; not a number gives 0"""
    if math.isnan(v):
        return 0
    p = float(np.rint(v))
    return int(min(max(p, 0.0), 255.0))


def vertex_color(p, normal, images, depth, k, w2c, centre, z_min=0.0, depth_tol=0.005, min_cos=0.2, power=2, mode=MODE_MEAN,
                 fill=(128, 128, 128)):
    """((r, g, b), views_used) of one vertex ``p`` (3 floats); ``normal`` 3 floats or None; ``images`` (n,H,W,3) uint8; ``depth``
    (n,H,W) float32 or None; ``k`` (n,3,3), ``w2c`` (n,4,4), ``centre`` (n,3) float64"""
    n, H, W = images.shape[:3]
    px, py, pz = (float(v) for v in p)
    A = [0.0, 0.0, 0.0]
    Wsum, best_w, best_s, used = 0.0, 0.0, None, 0
    one_tol = 1.0 + float(depth_tol)
    for v in range(n):
        if not _finite(px, py, pz):
            continue
        R, K, C = w2c[v], k[v], centre[v]
        c = [((float(R[i, 0]) * px + float(R[i, 1]) * py) + float(R[i, 2]) * pz) + float(R[i, 3]) for i in range(3)]
        if not _finite(*c) or not c[2] > z_min:
            continue
        q = [(float(K[i, 0]) * c[0] + float(K[i, 1]) * c[1]) + float(K[i, 2]) * c[2] for i in range(3)]
        with np.errstate(all="ignore"):
            x, y = float(np.float64(q[0]) / np.float64(q[2])), float(np.float64(q[1]) / np.float64(q[2]))
        if not _finite(x, y):
            continue
        x0, y0 = math.floor(x), math.floor(y)
        if not (0 <= x0 and x0 + 1 <= W - 1 and 0 <= y0 and y0 + 1 <= H - 1):
            continue
        fx, fy = x - float(x0), y - float(y0)
        cosv = 1.0
        if normal is not None:
            e = [px - float(C[0]), py - float(C[1]), pz - float(C[2])]
            ln = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            if ln == 0.0:
                continue                                        # the kernel's 0 / 0 is not a number, which fails cosv >= min_cos
            d = [e[0] / ln, e[1] / ln, e[2] / ln]
            cosv = abs((float(normal[0]) * d[0] + float(normal[1]) * d[1]) + float(normal[2]) * d[2])
            if not (cosv >= min_cos and cosv > 0.0):
                continue
        if depth is not None:
            D = [float(depth[v, y0 + j, x0 + i]) for j in (0, 1) for i in (0, 1)]   # float32 widened
            if not all(t > 0.0 for t in D):
                continue
            if not c[2] <= one_tol * min(D):
                continue
        w = 1.0
        for _ in range(int(power)):
            w = w * cosv
        s = []
        for ch in range(3):
            i00, i01 = float(images[v, y0, x0, ch]), float(images[v, y0, x0 + 1, ch])
            i10, i11 = float(images[v, y0 + 1, x0, ch]), float(images[v, y0 + 1, x0 + 1, ch])
            top = (1.0 - fx) * i00 + fx * i01
            bot = (1.0 - fx) * i10 + fx * i11
            s.append((1.0 - fy) * top + fy * bot)
        for ch in range(3):
            A[ch] = A[ch] + w * s[ch]
        Wsum = Wsum + w
        if used == 0 or w > best_w:
            best_w, best_s = w, s
        used += 1
    if used == 0:
        return tuple(int(f) for f in fill), 0
    if mode == MODE_BEST:
        return tuple(_to_byte(v) for v in best_s), used
    with np.errstate(all="ignore"):
        return tuple(_to_byte(float(np.float64(a) / np.float64(Wsum))) for a in A), used


def vertex_colors(verts, normals, images, depth, k, w2c, centre, **kw):
    """``vertex_color`` over a mesh: colors (V,3) uint8, views_used (V,) uint8"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    images = np.asarray(images, np.uint8)
    depth = None if depth is None else np.asarray(depth, np.float32)
    k, w2c, centre = np.asarray(k, np.float64), np.asarray(w2c, np.float64), np.asarray(centre, np.float64)
    colors = np.zeros((len(verts), 3), np.uint8)
    used = np.zeros(len(verts), np.uint8)
    for i, p in enumerate(verts):
        colors[i], used[i] = vertex_color(p, None if normals is None else normals[i], images, depth, k, w2c, centre, **kw)
    return colors, used


def _mean_half_even(total, count):
    q, r = total // count, total % count
    return q + (1 if 2 * r > count or (2 * r == count and q % 2 == 1) else 0)


def fill_round(faces, colors, state):
    """One Jacobi round: (colors (V,3) uint8, state (V,) uint8, filled).  An empty vertex (state 0) walks its corner slots 3f + e
    in ascending order and visits corners (e + 1) % 3 and (e + 2) % 3 of face f; the coloured ones are averaged in integers,
    half to even.  A neighbour shared by two faces is visited twice."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    colors = np.asarray(colors, np.uint8)
    state = np.asarray(state, np.uint8)
    V = len(state)
    out_c, out_s, filled = colors.copy(), state.copy(), 0
    flat = faces.reshape(-1)
    for v in range(V):
        if state[v] != 0:
            continue
        tot, count = [0, 0, 0], 0
        for slot in np.nonzero(flat == v)[0]:                  # ascending slot order
            f, e = divmod(int(slot), 3)
            for j in (1, 2):
                u = int(faces[f, (e + j) % 3])
                if u < 0 or u >= V or state[u] == 0:
                    continue
                for ch in range(3):
                    tot[ch] += int(colors[u, ch])
                count += 1
        if count > 0:
            out_c[v] = [_mean_half_even(t, count) for t in tot]
            out_s[v] = 1
            filled += 1
    return out_c, out_s, filled


def fill(faces, colors, views_used, rounds):
    """Up to ``rounds`` rounds, ending after a round that fills nothing (which is counted): (colors, state, rounds_run)"""
    colors = np.asarray(colors, np.uint8).copy()
    state = (np.asarray(views_used) != 0).astype(np.uint8)
    run = 0
    if len(np.asarray(faces).reshape(-1, 3)) == 0:
        return colors, state, 0
    while run < rounds:
        colors, state, filled = fill_round(faces, colors, state)
        run += 1
        if filled == 0:
            break
    return colors, state, run


def projection_camera(K, c2w):
    """(k, w2c, centre) float64 of intrinsics ``K`` and a camera-to-world matrix: the host arrays ``vertex_colors`` takes"""
    K = np.asarray(K, np.float64)
    c2w = np.asarray(c2w, np.float64)
    return K / K[2, 2], np.linalg.inv(c2w), c2w[:3, 3].copy()


# ------------------------------------------------------------------ scenes the tests share
def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(verts (V,3) float64, faces (F,3) int32) of an icosahedron subdivided ``level`` times: 10 * 4^level + 2 vertices (642
    at level 3, 2562 at level 4), outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.asarray(v, np.float64) * radius + np.asarray(centre, np.float64), np.asarray(f, np.int32)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """camera-to-world 4x4 float64 (x right, y down, z forward) of a camera at ``eye`` that looks at ``target``"""
    eye = np.asarray(eye, np.float64)
    z = np.asarray(target, np.float64) - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    return c2w


def ring_cameras(n, distance, height=0.0, phase=0.1):
    """``n`` camera-to-world matrices on a ring round the z axis, each looking at the origin"""
    out = []
    for i in range(n):
        a = phase + 2.0 * np.pi * i / n
        out.append(look_at((distance * np.cos(a), distance * np.sin(a), height)))
    return np.stack(out)


def intrinsics(H, W, focal):
    """3x3 float64 with the principal point at the centre of the pixel grid (pixel centres are the integers)"""
    return np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def cam_file_text(K, E):
    """the text of a ``*_cam.txt`` with extrinsics ``E`` (world to camera) and intrinsics ``K``"""
    lines = ["extrinsic"] + [" ".join(repr(float(v)) for v in row) for row in np.asarray(E)] + ["", "intrinsic"]
    lines += [" ".join(repr(float(v)) for v in row) for row in np.asarray(K)] + ["", "425.0 2.5", ""]
    return "\n".join(lines)


def write_dtu_tree(root, scans, views, K, c2ws, pictures):
    """``<root>/cameras/{:0>8}_cam.txt`` and ``<root>/scan<N>/image/{:0>6}.png`` for every scan and view; ``pictures[scan][i]``
    is the (H,W,3) uint8 picture of view ``views[i]``"""
    from PIL import Image

    os.makedirs(os.path.join(root, "cameras"), exist_ok=True)
    for v, c2w in zip(views, c2ws):
        with open(os.path.join(root, "cameras", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write(cam_file_text(K, np.linalg.inv(c2w)))
    for scan in scans:
        os.makedirs(os.path.join(root, "scan%d" % scan, "image"), exist_ok=True)
        for i, v in enumerate(views):
            Image.fromarray(pictures[scan][i]).save(os.path.join(root, "scan%d" % scan, "image", "{:0>6}.png".format(v)))
