"""The numpy statement of mesh smoothing (smooth_ref.py) checked on its own, on the host: what Taubin and Laplacian steps do
to a noisy sphere, that cotangent weights leave a planar triangulation alone where uniform weights do not, that they move a
cube's irregular tessellation less, and the edges of the rule (dead faces, the border, pinning, the factors).  The device is
compared with this statement bit for bit in test_gpu_smooth_mesh.py."""
import functools

import numpy as np
import pytest

import simplify_ref as S
import smooth_ref as R

WEIGHTS = ("cotangent", "uniform")


@functools.lru_cache(maxsize=None)
def noisy_sphere(level):
    v, f = S.icosphere(level)                                # unit radius
    return v * (1.0 + 0.01 * np.random.default_rng(0).standard_normal(len(v)))[:, None], f


def radial(v):
    """the mean radius, and the rms of the radii about that mean"""
    r = np.linalg.norm(v, axis=1)
    return float(r.mean()), float(r.std())


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("level", [3, 4])
def test_noisy_icosphere(level, weights):
    v, f = noisy_sphere(level)
    assert len(v) == {3: 642, 4: 2562}[level]
    _, rms_in = radial(v)
    lap = R.smooth(v, f, method="laplacian", weights=weights, iterations=10)
    tau = R.smooth(v, f, method="taubin", weights=weights, iterations=10)
    assert not lap["border"].any() and not tau["border"].any()          # a closed manifold
    mean_l, rms_l = radial(lap["verts"])
    mean_t, rms_t = radial(tau["verts"])
    print(level, weights, "laplacian", mean_l, rms_l, "taubin", mean_t, rms_t, "input rms", rms_in)
    assert abs(mean_t - 1.0) < 0.005                                    # Taubin does not shrink
    assert mean_l < 0.99                                                # Laplacian does
    assert rms_t < 0.5 * rms_in and rms_l < 0.5 * rms_in


def test_jittered_planar_lattice():
    v, f = R.lattice(12)
    moved = {}
    for weights in WEIGHTS:
        out = R.smooth(v, f, method="laplacian", weights=weights, iterations=1)
        assert int(out["border"].sum()) == 44
        assert np.array_equal(out["verts"][out["border"] != 0], v[out["border"] != 0])
        assert (out["verts"][:, 2] == 0.0).all()
        moved[weights] = float(np.linalg.norm(out["verts"] - v, axis=1).max())
    _, _, _, wa, wb = R.rows(v, f, "cotangent")
    print("cotangent weights", wa.min(), wa.max(), wb.min(), wb.max(), "moved", moved)
    assert min(wa.min(), wb.min()) > 0.0 and max(wa.max(), wb.max()) < 64.0     # every angle acute: nothing is clamped
    assert moved["cotangent"] <= 1e-12
    assert moved["uniform"] > 1e-2


def test_cube_cotangent_moves_less_than_uniform():
    v, f = S.cube()
    moved = {w: float(np.linalg.norm(R.smooth(v, f, weights=w, iterations=10)["verts"] - v, axis=1).max()) for w in WEIGHTS}
    print(moved)
    assert 0.0 < moved["cotangent"] < moved["uniform"]


def tetrahedron():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) + 0.125
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


@pytest.mark.parametrize("weights", WEIGHTS)
def test_a_dead_face_contributes_nothing(weights):
    v, f = tetrahedron()
    want = R.smooth(v, f, weights=weights, iterations=3)
    dead = np.array([[0, 0, 1], [2, 3, 2], [1, 1, 1]], np.int32)
    got = R.smooth(v, np.concatenate([dead[:1], f, dead[1:]]), weights=weights, iterations=3)
    assert got["verts"].tobytes() == want["verts"].tobytes() and np.array_equal(got["border"], want["border"])
    assert not (got["verts"] == v).all()


def test_a_zero_area_face_is_dead_under_cotangent_only():
    v, f = tetrahedron()
    v = np.concatenate([v, [(v[0] + v[1]) / 2]])              # vertex 4 on the edge 0-1; the face (0, 1, 4) has no area
    f2 = np.concatenate([f, [[0, 1, 4]]]).astype(np.int32)
    cot = R.smooth(v, f2, weights="cotangent", iterations=2, boundary="free")
    assert cot["verts"][:4].tobytes() == R.smooth(v[:4], f, weights="cotangent", iterations=2)["verts"].tobytes()
    assert cot["verts"][4].tobytes() == v[4].tobytes() and not cot["border"].any()
    uni = R.smooth(v, f2, weights="uniform", iterations=2, boundary="free")
    assert uni["border"][[0, 1, 4]].all() and not (uni["verts"][4] == v[4]).all()


def test_a_vertex_without_faces_keeps_its_bits():
    v, f = tetrahedron()
    v = np.concatenate([v, [[0.1, np.pi, -7.0]]])
    for weights in WEIGHTS:
        out = R.smooth(v, f, weights=weights, boundary="free")
        assert out["verts"][4].tobytes() == v[4].tobytes() and out["border"][4] == 0


def test_an_edge_of_three_faces_marks_both_ends():
    v, f = tetrahedron()
    v = np.concatenate([v, [[0.7, 0.6, -0.5]]])
    out = R.smooth(v, np.concatenate([f, [[0, 1, 4]]]).astype(np.int32), weights="uniform", iterations=1)
    assert out["border"].tolist() == [1, 1, 0, 0, 1]          # 0 and 1: the edge of three faces; 4: two open edges
    assert np.array_equal(out["verts"][[0, 1, 4]], v[[0, 1, 4]]) and not (out["verts"][[2, 3]] == v[[2, 3]]).all()


def test_boundary_free_moves_the_border_and_pinned_holds():
    v, f = R.lattice(6)
    fixed = R.smooth(v, f, weights="uniform", iterations=2)
    free = R.smooth(v, f, weights="uniform", iterations=2, boundary="free")
    b = fixed["border"] != 0
    assert b.sum() == 20 and np.array_equal(fixed["border"], free["border"])
    assert np.array_equal(fixed["verts"][b], v[b]) and (np.abs(free["verts"][b] - v[b]).max(1) > 0).all()
    pinned = np.zeros(len(v), np.uint8)
    pinned[[14, 15, 0]] = 1
    out = R.smooth(v, f, weights="uniform", iterations=2, boundary="free", pinned=pinned)
    assert out["verts"][pinned != 0].tobytes() == v[pinned != 0].tobytes()
    assert (np.abs(out["verts"][pinned == 0] - v[pinned == 0]).max(1) > 0).all()
    assert not np.array_equal(out["verts"][16], free["verts"][16])      # a held neighbour changes what 16 sees in step 2


def test_iterations_zero_and_the_default_mu():
    v, f = noisy_sphere(3)
    for method in ("taubin", "laplacian"):
        assert R.smooth(v, f, method=method, iterations=0)["verts"].tobytes() == v.tobytes()
    assert R.default_mu(0.5) == 1 / (0.1 - 2) and abs(R.default_mu(0.5) + 0.5263157894736842) < 1e-15
    assert R.factors("taubin", 2) == [0.5, 1 / (0.1 - 2)] * 2 and R.factors("laplacian", 3, lam=1.0) == [1.0] * 3
    a = R.smooth(v, f, iterations=3)["verts"]
    assert a.tobytes() == R.smooth(v, f, iterations=3, mu=1 / (0.1 - 2))["verts"].tobytes()
    assert a.tobytes() != R.smooth(v, f, iterations=3, mu=-0.6)["verts"].tobytes()


def test_a_step_sums_in_ascending_slot_order():
    # the statement against a plain loop over the sorted slots, one vertex at a time
    v, f = S.soup(40, 90, seed=5)
    for weights in WEIGHTS:
        r = R.rows(v, f, weights)
        got = R.step(v, 0.5, r, np.zeros(len(v), bool))
        rv, ra, rb, wa, wb = r
        for x in range(len(v)):
            num, den = np.zeros(3), np.float64(0.0)
            for i in np.flatnonzero(rv == x):
                num = num + (wa[i] * (v[ra[i]] - v[x]) + wb[i] * (v[rb[i]] - v[x]))
                den = den + (wa[i] + wb[i])
            want = v[x] + (np.float64(0.5) * num) / den if den > 0 else v[x]
            assert got[x].tobytes() == want.tobytes(), (weights, x)
