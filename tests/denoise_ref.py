"""The numpy statement of mesh denoising (include/ufr.h, "mesh denoising"; uforecon_amd/csrc/mesh_denoise.hip): the bilateral
normal filter of Zheng et al. 2011 (local, iterative) with the vertex update of Sun et al. 2007.  Every product, quotient and
sum is a statement of its own; the work is vectorised over faces (or vertices) and LOOPS over the neighbour position, so
every sum runs in the order the header states -- self first, then the three corner runs in ascending slot -- and the device's
bits can be asked for.  The fixtures are simplify_ref's and smooth_ref's."""
import numpy as np

SIGMA_R = 0.35                     # the chord of about 20 degrees: a neighbour turned that far weighs e^-1/2


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def k(u):
    """stands in for exp(-u): (1 - u / 256)^256 by eight squarings, 0 from u = 256 on and for a NaN"""
    with np.errstate(all="ignore"):
        x = 1.0 - np.asarray(u, np.float64) / 256.0
        x = np.where(x > 0.0, x, 0.0)
        for _ in range(8):
            x = x * x
    return x


def mean_edge_length(verts, faces):
    """the default sigma_s: the mean of the three edge lengths of every live face (float64 on the host)"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(all="ignore"):
        nf = np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
    live = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]) & (nf > 0) & np.isfinite(nf)
    edges = np.stack([p1 - p0, p2 - p1, p0 - p2])[:, live]
    return float(np.mean(np.linalg.norm(edges, axis=-1)))


def face_records(verts, faces):
    """(live (F,) bool, n (F,3), A (F,), c (F,3)) from the positions given; a dead face has zeros"""
    F = len(faces)
    p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    u, t = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        m = np.stack([u[:, 1] * t[:, 2] - u[:, 2] * t[:, 1], u[:, 2] * t[:, 0] - u[:, 0] * t[:, 2],
                      u[:, 0] * t[:, 1] - u[:, 1] * t[:, 0]], 1).reshape(F, 3)
        nf = np.sqrt(_dot(m, m))
        live = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]) & (nf > 0.0) & np.isfinite(nf)
        safe = np.where(live, nf, 1.0)
        n = np.where(live[:, None], m / safe[:, None], 0.0)
        A = np.where(live, 0.5 * nf, 0.0)
        c = np.where(live[:, None], ((p0 + p1) + p2) / 3.0, 0.0)
    return live, n, A, c


def sorted_rows(V, faces):
    """(slots (3F,), runs (V+1,)): the corner slots sorted by the vertex they name (stable), and where every vertex's run starts"""
    corner = faces.reshape(-1)
    slots = np.argsort(corner, kind="stable")
    runs = np.searchsorted(corner[slots], np.arange(V + 1))
    return slots, runs


def neighbourhood_steps(faces, live, slots, runs):
    """yields (f_idx, g_idx) pairs of equal length, one per neighbour position: first every live face with itself, then, for
    corner e and row position j of the corner vertex's run, the faces whose row there is a neighbour, with that neighbour.
    Walking the yields in order visits every face's neighbourhood in the header's order."""
    F = len(faces)
    mine = np.flatnonzero(live)
    yield mine, mine
    for e in range(3):
        v = faces[mine, e]
        start, length = runs[v], runs[v + 1] - runs[v]
        for j in range(int(length.max()) if len(mine) else 0):
            has = j < length
            f = mine[has]
            g = slots[start[has] + j] // 3
            keep = (g != f) & live[g]
            for ep in range(e):
                keep &= ~(faces[g] == faces[f, ep][:, None]).any(1)
            yield f[keep], g[keep]
    assert F == len(live)


def neighbourhoods(faces, live, slots, runs):
    """the same as lists, one per face (a dead face: an empty list); for the tests of the statement"""
    out = [[] for _ in range(len(faces))]
    for f, g in neighbourhood_steps(faces, live, slots, runs):
        for a, b in zip(f.tolist(), g.tolist()):
            out[a].append(b)
    return out


def normal_step(n, A, c, live, faces, slots, runs, two_ss, two_rr):
    acc = np.zeros_like(n)
    with np.errstate(all="ignore"):
        for f, g in neighbourhood_steps(faces, live, slots, runs):
            dc, dn = c[g] - c[f], n[g] - n[f]
            w = (A[g] * k(_dot(dc, dc) / two_ss)) * k(_dot(dn, dn) / two_rr)
            acc[f] = acc[f] + w[:, None] * n[g]
        L = np.sqrt(_dot(acc, acc))
        ok = live & (L > 0.0) & np.isfinite(L)
        return np.where(ok[:, None], acc / np.where(ok, L, 1.0)[:, None], n)


def vertex_step(q, n, live, faces, slots, runs, held):
    V = len(q)
    s, cnt = np.zeros_like(q), np.zeros(V)
    length = runs[1:] - runs[:-1]
    with np.errstate(all="ignore"):
        for j in range(int(length.max()) if V else 0):
            v = np.flatnonzero(j < length)
            g = slots[runs[v] + j] // 3
            v, g = v[live[g]], g[live[g]]
            cg = ((q[faces[g, 0]] + q[faces[g, 1]]) + q[faces[g, 2]]) / 3.0
            d = _dot(cg - q[v], n[g])
            s[v] = s[v] + n[g] * d[:, None]
            cnt[v] = cnt[v] + 1.0
        move = (cnt > 0.0) & ~held
        return np.where(move[:, None], q + s / np.where(move, cnt, 1.0)[:, None], q)


def border_of(V, faces, live):
    """(V,) uint8: some neighbour stands in the vertex's live rows a number of times other than 2"""
    f = faces[live]
    v = f.reshape(-1)
    a, b = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    pair, count = np.unique(np.concatenate([v * V + a, v * V + b]), return_counts=True)
    out = np.zeros(V, np.uint8)
    out[pair[count != 2] // V] = 1
    return out


def denoise(verts, faces, normal_iterations=5, vertex_iterations=10, sigma_s=None, sigma_r=SIGMA_R, boundary="fixed", pinned=None):
    """The outputs of ops.mesh_denoise as numpy arrays, in a dict of the same keys (``sigma_s`` None: the mean edge length)."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    V, F = len(verts), len(faces)
    assert boundary in ("fixed", "free") and normal_iterations >= 0 and vertex_iterations >= 0
    assert F == 0 or (faces.min() >= 0 and faces.max() < V)
    if V == 0 or F == 0:
        return dict(verts=verts.copy(), normals=np.zeros((F, 3)), border=np.zeros(V, np.uint8))
    sigma_s = mean_edge_length(verts, faces) if sigma_s is None else float(sigma_s)
    sigma_r = float(sigma_r)
    assert sigma_s > 0.0 and sigma_r > 0.0 and np.isfinite(sigma_s) and np.isfinite(sigma_r)
    two_ss, two_rr = np.float64(2.0 * (sigma_s * sigma_s)), np.float64(2.0 * (sigma_r * sigma_r))
    live, n, A, c = face_records(verts, faces)
    slots, runs = sorted_rows(V, faces)
    border = border_of(V, faces, live)
    held = np.zeros(V, bool)
    if boundary == "fixed":
        held |= border != 0
    if pinned is not None:
        pinned = np.asarray(pinned)
        assert pinned.shape == (V,) and pinned.dtype == np.uint8
        held |= pinned != 0
    for _ in range(int(normal_iterations)):
        n = normal_step(n, A, c, live, faces, slots, runs, two_ss, two_rr)
    q = verts.copy()
    for _ in range(int(vertex_iterations)):
        q = vertex_step(q, n, live, faces, slots, runs, held)
    return dict(verts=q, normals=n, border=border)
