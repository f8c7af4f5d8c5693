"""Mesh smoothing on the device (csrc/mesh_smooth.hip through ops.mesh_smooth): the positions and the border equal the numpy
statement (smooth_ref.py) bit for bit, and again on a rerun, on the fixtures test_smooth_ref.py checks the statement itself on;
argument errors, and the command end to end.  No tolerance anywhere: the header fixes the order of every operation.

Shapes: the icosphere at levels 3 and 4 spans 3 and 11 blocks of vertices and 15 and 60 of rows; the soups put the vertex and
row counts on both sides of a wave (64) and of a block (256) and bring dead faces, unreferenced vertices and high degrees; one
vertex named by 300 faces has a row run longer than a block, one named by 1300 a run longer than the chunk of rows the step
stages at a time; the rows of 256 icosphere vertices span two chunks.  1, 2 and 5 iterations end in either ping-pong buffer."""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import simplify_ref as S
import smooth_ref as R
from uforecon_amd import _lib, clean_mesh as CM, color_mesh as CMesh, dtu_eval, ops, simplify_mesh as SM, smooth_mesh as SMO
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

MODES = list(itertools.product(("taubin", "laplacian"), ("cotangent", "uniform"), ("fixed", "free")))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name.startswith("ico"):
        v, f = S.icosphere(int(name[3:]))
        return v * (1.0 + 0.01 * np.random.default_rng(0).standard_normal(len(v)))[:, None], f
    return {"cube": S.cube, "lattice": R.lattice, "patch": S.two_layer_patch, "slab": S.slab}[name]()


@functools.lru_cache(maxsize=None)
def want_of(name, method, weights, boundary, iterations):
    v, f = mesh(name)
    return R.smooth(v, f, method=method, weights=weights, iterations=iterations, boundary=boundary)


def device_run(v, f, pinned=None, **kw):
    out = ops.mesh_smooth(cuda(v), cuda(f), pinned=None if pinned is None else cuda(pinned), **kw)
    assert sorted(out) == ["border", "verts"]
    return {k: x.cpu().numpy() for k, x in out.items()}


def same(got, want):
    for k in ("verts", "border"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


def check(v, f, want=None, **kw):
    want = R.smooth(v, f, **kw) if want is None else want
    got = device_run(v, f, **kw)
    same(got, want)
    same(device_run(v, f, **kw), got)                    # a rerun gives the same bits
    return got


@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("method,weights,boundary", MODES)
@pytest.mark.parametrize("name", ["ico3", "ico4", "cube", "lattice", "patch", "slab"])
def test_bit_for_bit(name, method, weights, boundary, iterations):
    v, f = mesh(name)
    got = check(v, f, want_of(name, method, weights, boundary, iterations), method=method, weights=weights, boundary=boundary,
                iterations=iterations)
    closed = name in ("ico3", "ico4", "cube", "slab")            # the regular patch and the lattice under cotangent weights rest
    assert got["border"].any() != closed and (not closed or not np.array_equal(got["verts"], v))
    if boundary == "fixed":
        assert np.array_equal(got["verts"][got["border"] != 0], v[got["border"] != 0])
    if name == "lattice":
        assert int(got["border"].sum()) == 44 and (got["verts"][:, 2] == 0.0).all()


@pytest.mark.parametrize("V,F", [(n, n) for n in (1, 63, 64, 65, 255, 256, 257)] + [(257, 1), (3, 257), (64, 256)])
def test_counts_around_a_wave_and_a_block(V, F):
    v, f = S.soup(V, F, seed=V + F)
    for method, weights, boundary in MODES:
        check(v, f, method=method, weights=weights, boundary=boundary, iterations=2)
    pinned = (np.arange(V) % 3 == 0).astype(np.uint8)
    check(v, f, pinned=pinned, boundary="free", iterations=3)


@pytest.mark.parametrize("n", [300, 1300])
def test_a_row_run_longer_than_a_block_and_than_a_chunk(n):
    rng = np.random.default_rng(11)
    v = rng.random((700, 3))
    f = np.stack([np.zeros(n, np.int64), rng.integers(1, 700, n), rng.integers(1, 700, n)], 1)
    f = np.concatenate([np.roll(f[:100], 1, 1), f[100:200], np.roll(f[200:], 2, 1)]).astype(np.int32)   # vertex 0 at every corner
    assert (f == 0).sum() == n > ops.SMOOTH_BLOCK and (n > ops.SMOOTH_CHUNK) == (n == 1300)
    for weights in ("cotangent", "uniform"):
        got = check(v, f, weights=weights, boundary="free", iterations=3)
        assert not np.array_equal(got["verts"][0], v[0]) and got["border"][0] == 1


def test_zero_area_faces_pinned_and_iterations_zero():
    v, f = mesh("ico3")
    v = np.concatenate([v, [(v[f[0, 0]] + v[f[0, 1]]) / 2, [3.0, 3.0, 3.0]]])       # a vertex on an edge, a vertex without faces
    f = np.concatenate([f, [[f[0, 0], f[0, 1], len(v) - 2]], [[5, 5, 9]]]).astype(np.int32)
    pinned = np.zeros(len(v), np.uint8)
    pinned[::7] = 1
    for weights in ("cotangent", "uniform"):
        got = check(v, f, weights=weights, pinned=pinned, boundary="free", iterations=3)
        assert got["verts"][pinned != 0].tobytes() == v[pinned != 0].tobytes() and got["verts"][-1].tobytes() == v[-1].tobytes()
        zero = check(v, f, weights=weights, iterations=0)
        assert zero["verts"].tobytes() == v.tobytes()
    same(device_run(v, f, iterations=3), device_run(v, f, iterations=3, mu=1 / (0.1 - 2)))
    none = np.zeros((0, 3), np.int32)
    check(v, none)
    check(np.zeros((0, 3)), none)


def test_argument_errors_come_back_and_the_next_call_works():
    v, f = mesh("ico3")
    tv, tf = cuda(v), cuda(f)

    def bad(**kw):
        a = dict(verts=tv, faces=tf)
        a.update(kw)
        with pytest.raises(UfrError) as e:
            ops.mesh_smooth(**a)
        assert "\n" not in str(e.value).strip()

    fh, fl = tf.clone(), tf.clone()
    fh[3, 1], fl[0, 0] = len(v), -1
    ops.profile_enable(True)                             # every launch of the library is recorded from here on
    bad(faces=fh)
    bad(faces=fl)
    bad(lam=0.0)
    bad(lam=1.5)
    bad(mu=-0.5)                                         # mu == -lam
    bad(mu=0.3)
    bad(lam=0.8, mu=-0.7)
    bad(iterations=-1)
    bad(pinned=torch.zeros(len(v) - 1, dtype=torch.uint8, device="cuda"))
    bad(pinned=torch.zeros(len(v), dtype=torch.bool, device="cuda"))
    bad(verts=tv.float())
    bad(faces=tf.long())
    bad(method="umbrella")
    bad(weights="mean_value")
    bad(boundary="loose")
    bad(verts=tv.cpu())
    # the library itself refuses what ops refuses: straight through ctypes
    import ctypes as C

    lib = _lib.load()
    p, n = tv.data_ptr(), 1 << 20
    t = (C.c_double * 2)(0.5, float("nan"))
    assert lib.ufr_smooth_workspace_bytes(0, 4, 1) == 0 and lib.ufr_smooth_workspace_bytes(4, 2 ** 30, 1) == 0
    assert lib.ufr_smooth_workspace_bytes(4, 4, 2) == 0
    assert lib.ufr_smooth_workspace_bytes(4, 4, 1) > lib.ufr_smooth_workspace_bytes(4, 4, 0) >= 4 * 24
    assert lib.ufr_smooth_rows(p, p, 4, 4, p, p, 1, None, p, n, None) != 0 and b"null" in lib.ufr_last_error()
    assert lib.ufr_smooth_rows(p, p, 0, 4, p, p, 1, p, p, n, None) != 0
    assert lib.ufr_smooth_rows(p, p, 4, 4, p, p, 3, p, p, n, None) != 0 and b"weights" in lib.ufr_last_error()
    assert lib.ufr_smooth_rows(p, p, 4, 4, p, p, 1, p, p, 8, None) != 0 and b"workspace" in lib.ufr_last_error()
    assert lib.ufr_smooth_steps(4, 4, p, 1, None, None, t, 2, p, p + 4096, p, n, None) != 0 and b"finite" in lib.ufr_last_error()
    assert lib.ufr_smooth_steps(4, 4, p, 1, None, None, t, 1, p, p, p, n, None) != 0
    assert lib.ufr_smooth_steps(4, 4, p, 1, None, None, t, -1, p, p + 4096, p, n, None) != 0
    assert lib.ufr_smooth_steps(4, 4, p, 1, None, None, t, 1, p, p + 4096, p, 8, None) != 0
    launched = ops.profile_read()
    ops.profile_enable(False)
    assert launched == {}, launched
    same(device_run(v, f, iterations=2), want_of("ico3", "taubin", "cotangent", "fixed", 2))      # the next call works


def test_every_launch_is_profiled():
    v, f = mesh("ico3")
    ops.profile_enable(True)
    ops.mesh_smooth(cuda(v), cuda(f), iterations=3)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    assert {k: x["launches"] for k, x in prof.items()} == {"mesh_smooth_rows": 1, "mesh_smooth_border": 1, "mesh_smooth_step": 6}


def test_command_end_to_end(tmp_path, capsys):
    mesh_dir, out_dir = str(tmp_path / "mesh"), str(tmp_path / "smooth")
    os.makedirs(mesh_dir)
    v, f = mesh("ico4")
    colors = S.colors_of(len(v))
    CMesh.write_ply(os.path.join(mesh_dir, "scan7.ply"), v, f, colors)
    CM.write_ply(os.path.join(mesh_dir, "scan9.ply"), v, f)
    assert SMO.main(["--mesh_dir", mesh_dir, "--out_dir", out_dir, "--scans", "7", "8", "9", "--iterations", "4"]) == 0
    out = capsys.readouterr().out
    assert "scan8: no mesh at" in out
    report = json.load(open(os.path.join(out_dir, "smooth_mesh.json")))
    assert sorted(report) == ["scan7", "scan9"]
    v32 = v.astype(np.float32).astype(np.float64)        # what the PLY holds
    memory = SMO.smooth_mesh(v32, f, iterations=4)
    same(memory, R.smooth(v32, f, iterations=4))
    for name, has_colors in (("scan7", True), ("scan9", False)):
        ov, of, oc = dtu_eval.read_ply(os.path.join(out_dir, name + ".ply"), with_colors=True)
        r = report[name]
        assert sorted(r) == sorted(["mesh", "method", "weights", "iterations", "lam", "mu", "boundary", "vertices", "faces",
                                    "border_vertices", "mean_displacement", "max_displacement", "volume_in", "volume_out", "colors"])
        assert (r["vertices"], r["faces"], r["border_vertices"], r["colors"]) == (len(v), len(f), 0, has_colors)
        assert (r["method"], r["weights"], r["iterations"], r["lam"], r["mu"]) == ("taubin", "cotangent", 4, 0.5, 1 / (0.1 - 2))
        assert 0.0 < r["mean_displacement"] <= r["max_displacement"] < 0.05 and 4.0 < r["volume_out"] < 4.2 and r["volume_in"] > 4.0
        assert np.array_equal(of, f) and np.array_equal(ov, memory["verts"].astype(np.float32).astype(np.float64))
        assert (oc is not None) == has_colors and (oc is None or np.array_equal(oc, colors))
        assert "%s: %d vertices" % (name, len(v)) in out
        # the output goes on as it stands: the next stage takes it
        s = SM.simplify_mesh(ov, of, oc, cell=0.2)
        assert 0 < len(s["verts"]) < len(v) and (s["colors"] is not None) == has_colors
    # --ply, the other method, weights and boundary
    assert SMO.main(["--out_dir", out_dir, "--ply", os.path.join(mesh_dir, "scan9.ply"), "--method", "laplacian", "--weights", "uniform",
                     "--boundary", "free", "--iterations", "3", "--lam", "0.25"]) == 0
    ov, of = dtu_eval.read_ply(os.path.join(out_dir, "scan9.ply"))
    want = R.smooth(v32, f, method="laplacian", weights="uniform", boundary="free", iterations=3, lam=0.25)
    assert np.array_equal(ov, want["verts"].astype(np.float32).astype(np.float64)) and np.array_equal(of, f)
    assert json.load(open(os.path.join(out_dir, "smooth_mesh.json")))["scan9"]["mu"] is None
