"""The numpy statement of mesh smoothing (include/ufr.h, "mesh smoothing"; uforecon_amd/csrc/mesh_smooth.hip): Laplacian and
Taubin steps with uniform or cotangent weights, every product, quotient and sum a statement of its own, every sum left to right
(``np.add.at`` adds its rows one after the other, in the order given), so that the device's bits can be asked for.  Also the
planar lattice both test files share; the other fixtures are simplify_ref's."""
import numpy as np

MAX_WEIGHT = np.float64(64.0)      # the cotangent of a sliver angle under 0.9 degrees
PASS_BAND = 0.1                    # Taubin's k_pb


# ------------------------------------------------------------------ fixture
def lattice(n=12, jitter=0.15, seed=0):
    """an n x n equilateral lattice of spacing 1 in the plane z = 0, interior vertices moved by up to ``jitter`` along x and y.
    0.15 does not bound the angles below 90 degrees by itself; with seed 0 every angle stays acute at n = 12 (a property
    of this draw, which test_smooth_ref.py asserts), so no cotangent weight is clamped."""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    v = np.stack([ii + 0.5 * (jj % 2), jj * (np.sqrt(3.0) / 2.0), np.zeros((n, n))], -1).reshape(-1, 3)
    inner = ((ii > 0) & (ii < n - 1) & (jj > 0) & (jj < n - 1)).reshape(-1)
    v[inner, :2] += rng.uniform(-jitter, jitter, (n * n, 2))[inner]
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            f += [(a, b, c), (b, d, c)] if j % 2 == 0 else [(a, b, d), (a, d, c)]
    return v, np.asarray(f, np.int32)


# ------------------------------------------------------------------ the rule
def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def _clamp(w):
    w = np.where(w > 0.0, w, 0.0)
    return np.where(w > MAX_WEIGHT, MAX_WEIGHT, w)


def default_mu(lam):
    return 1.0 / (PASS_BAND - 1.0 / float(lam))


def factors(method="taubin", iterations=10, lam=0.5, mu=None):
    assert method in ("taubin", "laplacian") and int(iterations) == iterations and iterations >= 0 and 0.0 < lam <= 1.0
    if method == "laplacian":
        return [float(lam)] * int(iterations)
    mu = default_mu(lam) if mu is None else float(mu)
    assert mu < -lam
    return [float(lam), mu] * int(iterations)


def rows(verts, faces, weights="cotangent"):
    """The live rows in ascending slot: (v, a, b, wa, wb), each of one length.  Walking them in this order visits every
    vertex's rows in ascending slot, which is the order of the stable sort by vertex."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    V, F = len(verts), len(faces)
    assert F == 0 or (faces.min() >= 0 and faces.max() < V)
    live = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    nf = np.ones(F)
    if weights == "cotangent":
        p0 = verts[faces[:, 0]]
        u, t = verts[faces[:, 1]] - p0, verts[faces[:, 2]] - p0
        n0 = u[:, 1] * t[:, 2] - u[:, 2] * t[:, 1]
        n1 = u[:, 2] * t[:, 0] - u[:, 0] * t[:, 2]
        n2 = u[:, 0] * t[:, 1] - u[:, 1] * t[:, 0]
        with np.errstate(all="ignore"):
            nf = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        live &= (nf > 0.0) & np.isfinite(nf)
    else:
        assert weights == "uniform"
    slot = np.flatnonzero(np.repeat(live, 3))                # ascending s = 3f + e over the live faces
    f, e = slot // 3, slot % 3
    v, a, b = faces[f, e], faces[f, (e + 1) % 3], faces[f, (e + 2) % 3]
    if weights == "cotangent":
        pv, pa, pb = verts[v], verts[a], verts[b]
        with np.errstate(all="ignore"):
            wa = _clamp(_dot(pv - pb, pa - pb) / nf[f])      # the cotangent of the angle at b
            wb = _clamp(_dot(pv - pa, pb - pa) / nf[f])      # ... at a
    else:
        wa, wb = np.ones(len(slot)), np.ones(len(slot))
    return v, a, b, wa, wb


def border_of(V, v, a, b):
    """(V,) uint8: some neighbour stands in the vertex's live rows a number of times other than 2"""
    key = np.concatenate([v * V + a, v * V + b])
    pair, count = np.unique(key, return_counts=True)
    out = np.zeros(V, np.uint8)
    out[pair[count != 2] // V] = 1
    return out


def step(p, t, r, held):
    """one Jacobi step with factor t over the rows r; ``held`` (V,) bool stays"""
    v, a, b, wa, wb = r
    t = np.float64(t)
    num = np.zeros_like(p)
    den = np.zeros(len(p))
    pv = p[v]
    with np.errstate(all="ignore"):
        np.add.at(num, v, wa[:, None] * (p[a] - pv) + wb[:, None] * (p[b] - pv))
        np.add.at(den, v, wa + wb)
        move = (den > 0.0) & ~held
        new = p + (t * num) / np.where(move, den, 1.0)[:, None]
    return np.where(move[:, None], new, p)


def smooth(verts, faces, method="taubin", weights="cotangent", iterations=10, lam=0.5, mu=None, boundary="fixed", pinned=None):
    """The outputs of ops.mesh_smooth as numpy arrays, in a dict of the same keys."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    V = len(verts)
    assert boundary in ("fixed", "free")
    ts = factors(method, iterations, lam, mu)
    r = rows(verts, faces, weights)
    border = border_of(V, r[0], r[1], r[2])
    held = np.zeros(V, bool)
    if boundary == "fixed":
        held |= border != 0
    if pinned is not None:
        pinned = np.asarray(pinned)
        assert pinned.shape == (V,) and pinned.dtype == np.uint8
        held |= pinned != 0
    p = verts.copy()
    for t in ts:
        p = step(p, t, r, held)
    return dict(verts=p, border=border)
