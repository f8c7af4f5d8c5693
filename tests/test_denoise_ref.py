"""The numpy statement of mesh denoising (denoise_ref.py) checked on its own, on the host: the weight kernel against exp, the
order of a face's neighbourhood, what the filter does to a noisy cube and a noisy sphere beside Taubin smoothing (the measured
values are in DESIGN.md 3.4.16), held vertices, the border, the header's section and the command's argument errors.  The
device is compared with this statement bit for bit in test_gpu_denoise_mesh.py."""
import functools
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import simplify_ref as S
import smooth_ref as R
from uforecon_amd import _lib, denoise_mesh as DM, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parts(v, f):
    f = np.asarray(f).astype(np.int64)
    live, n, A, c = D.face_records(np.asarray(v, np.float64), f)
    slots, runs = D.sorted_rows(len(v), f)
    return f, live, n, A, c, slots, runs


def test_weight_kernel_stands_in_for_exp():
    u = np.linspace(0.0, 300.0, 300001)
    err = np.abs(D.k(u) - np.exp(-u))
    print("largest difference", err.max(), "at u =", u[err.argmax()])
    assert err.max() < 2e-3
    assert D.k(0.0) == 1.0 and 0.0 < D.k(200.0) < 1e-160
    assert (D.k(np.array([256.0, 257.0, 1e300, np.inf, np.nan])) == 0.0).all()
    x = np.float64(1.0 - 1.5 / 256.0)
    for _ in range(8):
        x = x * x
    assert D.k(1.5) == x


def test_neighbourhood_on_the_cube_is_the_faces_sharing_a_vertex():
    v, f = S.cube()
    f64, live, *_, slots, runs = parts(v, f)
    assert live.all()
    nb = D.neighbourhoods(f64, live, slots, runs)
    by_vertex = [set() for _ in range(len(v))]
    for i, tri in enumerate(f64.tolist()):
        for x in tri:
            by_vertex[x].add(i)
    for i, tri in enumerate(f64.tolist()):
        assert nb[i][0] == i
        assert len(nb[i]) == len(set(nb[i]))                                # each once
        assert set(nb[i]) == by_vertex[tri[0]] | by_vertex[tri[1]] | by_vertex[tri[2]]
        first = sorted(by_vertex[tri[0]] - {i})                              # corner 0's run, ascending slot = ascending face
        assert nb[i][1:1 + len(first)] == first


def test_neighbourhood_of_a_quad_by_hand():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    f64, live, *_, slots, runs = parts(v, f)
    assert D.neighbourhoods(f64, live, slots, runs) == [[0, 1], [1, 0]]     # the shared edge counts once
    # a third face at vertex 2 only, a dead face at vertex 0, and the order: self, corner 0's run, corner 1's, corner 2's
    f = np.array([[0, 1, 2], [0, 0, 3], [0, 2, 3], [2, 4, 1]], np.int32)
    f64, live, *_, slots, runs = parts(v, f)
    assert live.tolist() == [True, False, True, True]
    nb = D.neighbourhoods(f64, live, slots, runs)
    assert nb == [[0, 2, 3], [], [2, 0, 3], [3, 0, 2]]
    # ... face 0 = (0, 1, 2): corner 0 (vertex 0) reaches 2; corner 1 (vertex 1) reaches 3; corner 2 (vertex 2) reaches 2 and 3 again
    f = np.array([[1, 2, 0], [0, 2, 3], [2, 4, 1]], np.int32)
    f64, live, *_, slots, runs = parts(v, f)
    assert D.neighbourhoods(f64, live, slots, runs)[0] == [0, 2, 1]         # vertex 1 first, so face 2 comes before face 1


def face_normals(v, f):
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n / np.linalg.norm(n, axis=1)[:, None]


def cube_distance(x):
    """the distance of every point to the surface of the unit cube"""
    outside = np.linalg.norm(np.maximum(np.maximum(-x, x - 1.0), 0.0), axis=1)
    inside = np.minimum(x, 1.0 - x).min(1)
    return np.where(outside > 0.0, outside, np.maximum(inside, 0.0))


@functools.lru_cache(maxsize=None)
def noisy_cube(n):
    v, f = S.cube(n)
    return v, v + 0.01 * np.random.default_rng(0).standard_normal(v.shape), f


@pytest.mark.parametrize("n", [9, 17])
def test_noisy_cube_keeps_its_creases(n):
    clean, v, f = noisy_cube(n)
    true = face_normals(clean, f)

    def angle(x):
        return float(np.degrees(np.arccos(np.clip((face_normals(x, f) * true).sum(1), -1.0, 1.0))).mean())

    out = D.denoise(v, f)
    tau = R.smooth(v, f)["verts"]
    a_in, a_tau, a_out = angle(v), angle(tau), angle(out["verts"])
    d_in, d_tau, d_out = (float(cube_distance(x).mean()) for x in (v, tau, out["verts"]))
    print(n, "normal error: input %.3f taubin %.3f this %.3f degrees; distance: input %.5f taubin %.5f this %.5f" % (
        a_in, a_tau, a_out, d_in, d_tau, d_out))
    assert a_out < 0.5 * min(a_in, a_tau)
    assert d_out < d_in and d_out < d_tau
    assert not out["border"].any() and out["normals"].shape == (len(f), 3)
    assert np.abs(np.linalg.norm(out["normals"], axis=1) - 1.0).max() < 1e-15


def test_noisy_icosphere_does_not_shrink():
    v, f = S.icosphere(3)
    v = v * (1.0 + 0.01 * np.random.default_rng(0).standard_normal(len(v)))[:, None]
    rms_in = np.linalg.norm(v, axis=1).std()

    def radial(x):
        r = np.linalg.norm(x, axis=1)
        return float(r.mean()), float(r.std() / rms_in)

    mean_in = radial(v)[0]
    mean_out, left_out = radial(D.denoise(v, f)["verts"])
    mean_tau, left_tau = radial(R.smooth(v, f)["verts"])
    print("mean radius: input %.4f this %.4f taubin %.4f; noise left: this %.3f taubin %.3f" % (mean_in, mean_out, mean_tau, left_out, left_tau))
    assert abs(mean_out - mean_in) < abs(mean_tau - mean_in)
    assert left_out < left_tau


def test_held_vertices_keep_their_bits():
    v, f = R.lattice(8)
    v = v + 0.05 * np.random.default_rng(3).standard_normal(v.shape)
    fixed = D.denoise(v, f, sigma_r=1.0)
    b = fixed["border"] != 0
    assert b.sum() == 28 and fixed["verts"][b].tobytes() == v[b].tobytes()
    assert (np.abs(fixed["verts"][~b] - v[~b]).max(1) > 0).all()
    free = D.denoise(v, f, sigma_r=1.0, boundary="free")
    assert np.array_equal(free["border"], fixed["border"]) and (np.abs(free["verts"][b] - v[b]).max(1) > 0).all()
    pinned = np.zeros(len(v), np.uint8)
    pinned[[0, 27, 28]] = 1
    out = D.denoise(v, f, sigma_r=1.0, boundary="free", pinned=pinned)
    assert out["verts"][pinned != 0].tobytes() == v[pinned != 0].tobytes()
    assert (np.abs(out["verts"][pinned == 0] - v[pinned == 0]).max(1) > 0).all()
    assert out["normals"].tobytes() == free["normals"].tobytes()           # the normals do not see who is held
    # no vertex steps: the input's bits; no normal steps: the faces' own normals
    assert D.denoise(v, f, vertex_iterations=0)["verts"].tobytes() == v.tobytes()
    own = D.denoise(v, f, normal_iterations=0)["normals"]
    assert own.tobytes() == D.face_records(v, f.astype(np.int64))[1].tobytes()
    assert np.abs(own - face_normals(v, f)).max() < 1e-15


@pytest.mark.parametrize("name", ["lattice", "patch", "soup"])
def test_border_is_the_border_of_cotangent_smoothing(name):
    v, f = {"lattice": R.lattice, "patch": S.two_layer_patch, "soup": lambda: S.soup(60, 150, seed=2)}[name]()
    want = R.smooth(v, f, weights="cotangent", iterations=0)["border"]
    got = D.denoise(v, f, 1, 1)["border"]
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.any()


def test_dead_faces_are_nobodys_neighbour():
    v, f = S.icosphere(2)
    v = v * (1.0 + 0.01 * np.random.default_rng(0).standard_normal(len(v)))[:, None]
    want = D.denoise(v, f, 2, 2, sigma_s=0.3)
    v2 = np.concatenate([v, [v[f[0, 0]], [3.0, 3.0, 3.0]]])                       # a second vertex at the place of another
    dead = np.array([[f[0, 0], len(v), f[0, 1]], [5, 5, 9]], np.int32)           # no area (an edge of length 0); a vertex named twice
    f2 = np.concatenate([dead[:1], f, dead[1:]]).astype(np.int32)
    got = D.denoise(v2, f2, 2, 2, sigma_s=0.3, boundary="free")
    assert got["verts"][:len(v)].tobytes() == want["verts"].tobytes() and got["verts"][len(v):].tobytes() == v2[len(v):].tobytes()
    assert got["normals"][1:-1].tobytes() == want["normals"].tobytes() and not got["normals"][[0, -1]].any()
    assert not got["border"].any()


def test_default_sigma_s_is_the_mean_edge_length():
    v, f = S.cube()
    want = np.mean([np.linalg.norm(v[a] - v[b]) for tri in f.tolist() for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))])
    assert abs(D.mean_edge_length(v, f) - want) < 1e-15
    assert D.mean_edge_length(v, f) == DM.mean_edge_length(v, f)
    f2 = np.concatenate([f, [[3, 3, 70]]]).astype(np.int32)                         # a dead face has no edges
    assert D.mean_edge_length(v, f2) == D.mean_edge_length(v, f) == DM.mean_edge_length(v, f2)
    assert D.denoise(v, f, 1, 1)["verts"].tobytes() == D.denoise(v, f, 1, 1, sigma_s=D.mean_edge_length(v, f))["verts"].tobytes()
    assert D.SIGMA_R == DM.SIGMA_R == ops.DENOISE_SIGMA_R == 0.35


def test_header_section_and_signatures():
    import ctypes as C

    from uforecon_amd.build import SOURCES

    assert "mesh_denoise.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "uforecon_amd", "csrc", "mesh_denoise.hip"))
    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert text.count("/* ---- mesh denoising (ABI 507, additive) ----") == 1
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    smoothing = text[text.index("/* ---- mesh smoothing (ABI 507, additive)"):]
    assert smoothing.index("/* ----", 10) == smoothing.index("/* ---- mesh denoising (ABI 507, additive)")     # directly after smoothing
    section = text[text.index("mesh denoising (ABI 507, additive)"):]
    section = section[:section.index("/* ----", 10)]
    assert "mesh simplification" in text[text.index(section) + len(section):][:60]
    code = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    found = []
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code):
        found.append(name)
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is (C.c_size_t if res == "size_t" else C.c_int), name
        want = [p.strip() for p in params.split(",")]
        assert len(want) == len(args), name
        for p, a in zip(want, args):
            if "*" in p or p.startswith("ufr_stream"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}[p.split()[0]], (name, p)
    assert sorted(found) == ["ufr_denoise_faces", "ufr_denoise_normals", "ufr_denoise_vertices", "ufr_denoise_workspace_bytes"]
    assert sorted(found) == sorted(n for n in _lib.SIGNATURES if n.startswith("ufr_denoise_"))
    for phrase in ("Open3D and MeshLab were not compared", "sigma_r has to grow with the noise", "no real scan has been denoised",
                   "Only vertex positions change"):
        assert phrase in " ".join(section.replace(" * ", " ").split()), phrase


@pytest.mark.parametrize("argv", [["--sigma_s", "0"], ["--sigma_s", "-1"], ["--sigma_r", "0"], ["--sigma_r", "-0.35"], ["--sigma_r", "nan"],
                                  ["--normal_iterations", "-1"], ["--vertex_iterations", "-2"], ["--boundary", "loose"]])
def test_parser_errors(argv, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        DM.main(["--mesh_dir", str(tmp_path), "--out_dir", str(tmp_path / "out")] + argv)
    assert e.value.code == 2
    assert argv[0] in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")
