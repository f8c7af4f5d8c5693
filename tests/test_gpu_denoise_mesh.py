"""Mesh denoising on the device (csrc/mesh_denoise.hip through ops.mesh_denoise): positions, filtered normals and the border
equal the numpy statement (denoise_ref.py) bit for bit, and again on a rerun, on the fixtures test_denoise_ref.py checks the
statement itself on; argument errors, and the command end to end.  No tolerance anywhere: the header fixes the order of every
operation.

Shapes: the icosphere at level 4 spans 20 blocks of faces and 11 of vertices; the soups put the face and vertex counts on both
sides of a wave (64) and of a block (256) and bring dead faces, unreferenced vertices, high degrees and neighbour sums that
cancel; one vertex named by 300 faces has a row run, and so every one of those faces a neighbourhood, longer than a block,
one named by 1300 a run longer than the chunk of rows the vertex step stages at a time.  The iteration pairs end both phases
in either ping-pong buffer and leave either phase out."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import denoise_ref as D
import simplify_ref as S
import smooth_ref as R
from uforecon_amd import _lib, clean_mesh as CM, color_mesh as CMesh, denoise_mesh as DM, dtu_eval, ops, simplify_mesh as SM
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

ITERATIONS = [(1, 1), (2, 2), (5, 3), (0, 2), (2, 0), (0, 0)]
KEYS = ("verts", "normals", "border")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name.startswith("ico"):
        v, f = S.icosphere(int(name[3:]))
        return v * (1.0 + 0.01 * np.random.default_rng(0).standard_normal(len(v)))[:, None], f
    return {"cube": S.cube, "lattice": R.lattice, "patch": S.two_layer_patch, "slab": S.slab}[name]()


@functools.lru_cache(maxsize=None)
def sigma_of(name):
    v, f = mesh(name)
    return D.mean_edge_length(v, f)


@functools.lru_cache(maxsize=None)
def want_of(name, boundary, normal_iterations, vertex_iterations):
    v, f = mesh(name)
    return D.denoise(v, f, normal_iterations, vertex_iterations, sigma_s=sigma_of(name), boundary=boundary)


def device_run(v, f, pinned=None, **kw):
    out = ops.mesh_denoise(cuda(v), cuda(f), pinned=None if pinned is None else cuda(pinned), **kw)
    assert sorted(out) == sorted(KEYS)
    return {k: x.cpu().numpy() for k, x in out.items()}


def same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


def check(v, f, want=None, **kw):
    want = D.denoise(v, f, **kw) if want is None else want
    got = device_run(v, f, **kw)
    same(got, want)
    same(device_run(v, f, **kw), got)                    # a rerun gives the same bits
    return got


@pytest.mark.parametrize("boundary", ["fixed", "free"])
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("name", ["ico3", "ico4", "cube", "lattice", "patch", "slab"])
def test_bit_for_bit(name, iterations, boundary):
    v, f = mesh(name)
    nn, nv = iterations
    got = check(v, f, want_of(name, boundary, nn, nv), normal_iterations=nn, vertex_iterations=nv, sigma_s=sigma_of(name),
                boundary=boundary)
    closed = name in ("ico3", "ico4", "cube", "slab")
    assert got["border"].any() != closed
    if nv == 0:
        assert got["verts"].tobytes() == v.tobytes()
    if boundary == "fixed":
        assert got["verts"][got["border"] != 0].tobytes() == v[got["border"] != 0].tobytes()
    if name.startswith("ico") and nv:
        assert not np.array_equal(got["verts"], v)
    if name.startswith("ico"):
        own = want_of(name, boundary, 0, 0)["normals"]
        assert (got["normals"].tobytes() == own.tobytes()) == (nn == 0)
    if name == "lattice":
        assert int(got["border"].sum()) == 44


@pytest.mark.parametrize("V,F", [(n, n) for n in (1, 63, 64, 65, 255, 256, 257)] + [(257, 1), (3, 257), (64, 256)])
def test_counts_around_a_wave_and_a_block(V, F):
    v, f = S.soup(V, F, seed=V + F)
    for boundary in ("fixed", "free"):
        check(v, f, normal_iterations=2, vertex_iterations=2, sigma_s=0.4, boundary=boundary)
    pinned = (np.arange(V) % 3 == 0).astype(np.uint8)
    got = check(v, f, pinned=pinned, normal_iterations=3, vertex_iterations=3, sigma_s=0.4, sigma_r=0.7, boundary="free")
    assert got["verts"][pinned != 0].tobytes() == v[pinned != 0].tobytes()


def test_a_neighbour_sum_that_cancels_keeps_the_normal():
    # two faces over the same three vertices with opposite winding: equal areas and centroids, and a sigma_r at which
    # k(4 / two_rr) is exactly 1, so every step's sum is A n + A (-n) = 0 and the previous normal stays
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.3, 1.0]])
    f = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    assert D.k(4.0 / (2.0 * (1e10 * 1e10))) == 1.0
    got = check(v, f, normal_iterations=3, vertex_iterations=2, sigma_s=1.0, sigma_r=1e10, boundary="free")
    assert got["normals"].tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]
    # a soup of few vertices: most neighbourhoods are long, many faces dead
    v, f = S.soup(3, 257, seed=260)
    got = check(v, f, normal_iterations=2, vertex_iterations=1, sigma_s=0.5, sigma_r=1e6, boundary="free")
    live = np.linalg.norm(got["normals"], axis=1) > 0
    assert 0 < live.sum() < len(f)


@pytest.mark.parametrize("n", [300, 1300])
def test_a_row_run_longer_than_a_block_and_than_a_chunk(n):
    rng = np.random.default_rng(11)
    v = rng.random((700, 3))
    f = np.stack([np.zeros(n, np.int64), rng.integers(1, 700, n), rng.integers(1, 700, n)], 1)
    f = np.concatenate([np.roll(f[:100], 1, 1), f[100:200], np.roll(f[200:], 2, 1)]).astype(np.int32)   # vertex 0 at every corner
    assert (f == 0).sum() == n > ops.DENOISE_BLOCK and (n > ops.DENOISE_CHUNK) == (n == 1300)
    got = check(v, f, normal_iterations=2, vertex_iterations=3, sigma_s=0.5, sigma_r=0.8, boundary="free")
    assert not np.array_equal(got["verts"][0], v[0]) and got["border"][0] == 1


def test_dead_faces_a_vertex_without_faces_and_empty_inputs():
    v, f = mesh("ico3")
    v = np.concatenate([v, [v[f[0, 0]], [3.0, 3.0, 3.0]]])                       # a second vertex at the place of another; one without faces
    f = np.concatenate([[[f[0, 0], len(v) - 2, f[0, 1]]], f, [[5, 5, 9]]]).astype(np.int32)      # no area; a vertex named twice
    pinned = np.zeros(len(v), np.uint8)
    pinned[::7] = 1
    s = sigma_of("ico3")
    got = check(v, f, pinned=pinned, normal_iterations=2, vertex_iterations=3, sigma_s=s, boundary="free")
    assert got["verts"][pinned != 0].tobytes() == v[pinned != 0].tobytes() and got["verts"][-2:].tobytes() == v[-2:].tobytes()
    assert not got["normals"][[0, -1]].any() and (np.linalg.norm(got["normals"][1:-1], axis=1) > 0.99).all()
    assert not got["border"].any()
    inner = want_of("ico3", "free", 2, 3)                # the dead faces change nothing for the others
    assert got["normals"][1:-1].tobytes() == inner["normals"].tobytes()
    for nn, nv in ((0, 0), (0, 1), (1, 0)):
        check(v, f, normal_iterations=nn, vertex_iterations=nv, sigma_s=s)
    none = np.zeros((0, 3), np.int32)
    got = check(v, none, sigma_s=s)
    assert got["verts"].tobytes() == v.tobytes() and got["normals"].shape == (0, 3) and not got["border"].any()
    got = check(np.zeros((0, 3)), none, sigma_s=s)
    assert got["verts"].shape == (0, 3) and got["border"].shape == (0,)


@pytest.mark.parametrize("name", ["lattice", "patch", "ico3", "soup"])
def test_border_is_the_border_of_cotangent_smoothing(name):
    v, f = S.soup(200, 500, seed=4) if name == "soup" else mesh(name)
    want = ops.mesh_smooth(cuda(v), cuda(f), weights="cotangent", iterations=0)["border"]
    got = ops.mesh_denoise(cuda(v), cuda(f), 1, 1, sigma_s=0.5)["border"]
    assert got.dtype == torch.uint8 and torch.equal(got, want) and bool(want.any()) == (name != "ico3")


def test_argument_errors_come_back_and_the_next_call_works():
    v, f = mesh("ico3")
    tv, tf = cuda(v), cuda(f)

    def bad(**kw):
        a = dict(verts=tv, faces=tf, sigma_s=0.1)
        a.update(kw)
        with pytest.raises(UfrError) as e:
            ops.mesh_denoise(**a)
        assert "\n" not in str(e.value).strip()

    fh, fl = tf.clone(), tf.clone()
    fh[3, 1], fl[0, 0] = len(v), -1
    ops.profile_enable(True)                             # every launch of the library is recorded from here on
    bad(faces=fh)
    bad(faces=fl)
    bad(sigma_s=None)
    bad(sigma_s=0.0)
    bad(sigma_s=-1.0)
    bad(sigma_s=float("nan"))
    bad(sigma_s=float("inf"))
    bad(sigma_s=1e-200)                                  # its square is 0
    bad(sigma_r=0.0)
    bad(sigma_r=float("inf"))
    bad(normal_iterations=-1)
    bad(vertex_iterations=-1)
    bad(vertex_iterations=1.5)
    bad(pinned=torch.zeros(len(v) - 1, dtype=torch.uint8, device="cuda"))
    bad(pinned=torch.zeros(len(v), dtype=torch.bool, device="cuda"))
    bad(verts=tv.float())
    bad(faces=tf.long())
    bad(faces=tf[:, :2].contiguous())
    bad(boundary="loose")
    bad(verts=tv.cpu())
    # the library itself refuses what ops refuses: straight through ctypes
    lib = _lib.load()
    p, n = tv.data_ptr(), 1 << 20
    q = p + 4096
    nan, inf = float("nan"), float("inf")
    assert lib.ufr_denoise_workspace_bytes(0, 4) == 0 and lib.ufr_denoise_workspace_bytes(4, 2 ** 30) == 0
    assert lib.ufr_denoise_workspace_bytes(4, 0) == 0 and lib.ufr_denoise_workspace_bytes(-1, 4) == 0
    assert lib.ufr_denoise_workspace_bytes(4, 4) >= 4 * 188
    assert lib.ufr_denoise_faces(p, p, 4, 4, p, p, None, q, q, n, None) != 0 and b"null" in lib.ufr_last_error()
    assert lib.ufr_denoise_faces(p, p, 0, 4, p, p, q, q, q, n, None) != 0
    assert lib.ufr_denoise_faces(p, p, 4, 0, p, p, q, q, q, n, None) != 0
    assert lib.ufr_denoise_faces(p, p, 4, 4, p, p, p, q, q, n, None) != 0 and b"one buffer" in lib.ufr_last_error()
    assert lib.ufr_denoise_faces(p, p, 4, 4, p, p, q, q, q, 8, None) != 0 and b"workspace" in lib.ufr_last_error()
    for two_ss, two_rr, word in ((0.0, 1.0, b"two_ss"), (nan, 1.0, b"two_ss"), (inf, 1.0, b"two_ss"), (-1.0, 1.0, b"two_ss"),
                                 (1.0, 0.0, b"two_rr"), (1.0, nan, b"two_rr"), (1.0, -inf, b"two_rr")):
        assert lib.ufr_denoise_normals(p, 4, 4, p, two_ss, two_rr, 1, q, q, n, None) != 0 and word in lib.ufr_last_error()
    assert lib.ufr_denoise_normals(p, 4, 4, p, 1.0, 1.0, -1, q, q, n, None) != 0 and b"n_steps" in lib.ufr_last_error()
    assert lib.ufr_denoise_normals(p, 4, 4, p, 1.0, 1.0, 1, None, q, n, None) != 0
    assert lib.ufr_denoise_normals(p, 4, 4, p, 1.0, 1.0, 1, q, q, 8, None) != 0 and b"workspace" in lib.ufr_last_error()
    assert lib.ufr_denoise_vertices(4, 4, p, q, None, None, 1, p, p, q, n, None) != 0 and b"one buffer" in lib.ufr_last_error()
    assert lib.ufr_denoise_vertices(4, 4, p, p, None, None, 1, p, q, q, n, None) != 0 and b"one buffer" in lib.ufr_last_error()
    assert lib.ufr_denoise_vertices(4, 4, p, q, None, None, -1, p, p + 8192, q, n, None) != 0 and b"n_steps" in lib.ufr_last_error()
    assert lib.ufr_denoise_vertices(4, 4, p, q, None, None, 1, p, None, q, n, None) != 0 and b"null" in lib.ufr_last_error()
    assert lib.ufr_denoise_vertices(0, 4, p, q, None, None, 1, p, p + 8192, q, n, None) != 0
    assert lib.ufr_denoise_vertices(4, 4, p, q, None, None, 1, p, p + 8192, q, 8, None) != 0 and b"workspace" in lib.ufr_last_error()
    launched = ops.profile_read()
    ops.profile_enable(False)
    assert launched == {}, launched
    same(device_run(v, f, normal_iterations=2, vertex_iterations=2, sigma_s=sigma_of("ico3")), want_of("ico3", "fixed", 2, 2))


def test_every_launch_is_profiled():
    v, f = mesh("ico3")
    ops.profile_enable(True)
    ops.mesh_denoise(cuda(v), cuda(f), normal_iterations=3, vertex_iterations=4, sigma_s=0.1)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    assert {k: x["launches"] for k, x in prof.items()} == {"mesh_denoise_faces": 1, "mesh_denoise_rows": 1, "mesh_denoise_border": 1,
                                                           "mesh_denoise_normals": 3, "mesh_denoise_vertices": 4}


def test_command_end_to_end(tmp_path, capsys):
    mesh_dir, out_dir = str(tmp_path / "mesh"), str(tmp_path / "denoise")
    os.makedirs(mesh_dir)
    v, f = mesh("ico4")
    colors = S.colors_of(len(v))
    CMesh.write_ply(os.path.join(mesh_dir, "scan7.ply"), v, f, colors)
    CM.write_ply(os.path.join(mesh_dir, "scan9.ply"), v, f)
    CM.write_ply(os.path.join(mesh_dir, "scan10.ply"), v, np.zeros((0, 3), np.int32))
    assert DM.main(["--mesh_dir", mesh_dir, "--out_dir", out_dir, "--scans", "7", "8", "9", "10", "--normal_iterations", "3",
                    "--vertex_iterations", "4"]) == 0
    out = capsys.readouterr().out
    assert "scan8: no mesh at" in out and "scan10: " in out and "has no faces" in out
    report = json.load(open(os.path.join(out_dir, "denoise_mesh.json")))
    assert sorted(report) == ["scan7", "scan9"]
    v32 = v.astype(np.float32).astype(np.float64)        # what the PLY holds
    memory = DM.denoise_mesh(v32, f, normal_iterations=3, vertex_iterations=4)
    assert memory["sigma_s"] == D.mean_edge_length(v32, f)
    same(memory, D.denoise(v32, f, 3, 4))
    own = D.face_records(v32, f.astype(np.int64))[1]     # the mean angle between the faces' own normals and the filtered ones
    turn = float(np.degrees(np.arccos(np.clip((own * memory["normals"]).sum(1), -1.0, 1.0))).mean())
    assert turn > 1.0                                    # 1 % radial noise at edges of 0.077 tilts a face by several degrees
    for name, has_colors in (("scan7", True), ("scan9", False)):
        ov, of, oc = dtu_eval.read_ply(os.path.join(out_dir, name + ".ply"), with_colors=True)
        r = report[name]
        assert sorted(r) == sorted(["mesh", "normal_iterations", "vertex_iterations", "sigma_s", "sigma_r", "boundary", "vertices",
                                    "faces", "border_vertices", "mean_displacement", "max_displacement", "mean_normal_turn_deg",
                                    "volume_in", "volume_out", "colors"])
        assert (r["vertices"], r["faces"], r["border_vertices"], r["colors"]) == (len(v), len(f), 0, has_colors)
        assert (r["normal_iterations"], r["vertex_iterations"], r["sigma_r"], r["boundary"]) == (3, 4, 0.35, "fixed")
        assert r["sigma_s"] == memory["sigma_s"] and abs(r["mean_normal_turn_deg"] - turn) < 1e-6 * turn
        assert 0.0 < r["mean_displacement"] <= r["max_displacement"] < 0.05 and 4.0 < r["volume_out"] < 4.2 and r["volume_in"] > 4.0
        assert np.array_equal(of, f) and np.array_equal(ov, memory["verts"].astype(np.float32).astype(np.float64))
        assert (oc is not None) == has_colors and (oc is None or np.array_equal(oc, colors))
        assert "%s: %d vertices" % (name, len(v)) in out
        # the output goes on as it stands: the next stage takes it
        s = SM.simplify_mesh(ov, of, oc, cell=0.2)
        assert 0 < len(s["verts"]) < len(v) and (s["colors"] is not None) == has_colors
    # --ply, the sigmas and the other boundary
    assert DM.main(["--out_dir", out_dir, "--ply", os.path.join(mesh_dir, "scan9.ply"), "--boundary", "free", "--normal_iterations", "2",
                    "--vertex_iterations", "1", "--sigma_s", "0.08", "--sigma_r", "0.5"]) == 0
    ov, of = dtu_eval.read_ply(os.path.join(out_dir, "scan9.ply"))
    want = D.denoise(v32, f, 2, 1, sigma_s=0.08, sigma_r=0.5, boundary="free")
    assert np.array_equal(ov, want["verts"].astype(np.float32).astype(np.float64)) and np.array_equal(of, f)
    r = json.load(open(os.path.join(out_dir, "denoise_mesh.json")))["scan9"]
    assert (r["sigma_s"], r["sigma_r"], r["boundary"]) == (0.08, 0.5, "free")
