"""Mesh simplification on the device (csrc/mesh_simplify.hip through ops.mesh_simplify): every output equals the numpy statement
(simplify_ref.py) bit for bit, and again on a rerun, on the fixtures test_simplify_ref.py checks the statement itself on; target
mode, argument errors, and the command end to end.  No tolerance anywhere: the header fixes the order of every sum.

Shapes: the icosphere at levels 4 and 5 spans 11 and 41 blocks of vertices and 20 and 80 of faces; the soups put the vertex,
face, row and cluster counts on both sides of a wave (64) and of a block (256)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import color_mesh_ref as CR
import simplify_ref as R
from uforecon_amd import _lib, clean_mesh as CM, color_mesh as CMesh, dtu_eval, ops, simplify_mesh as SM
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

ARRAYS = ("verts", "faces", "colors", "vertex_map", "face_map", "placed", "count")
NUMBERS = ("cell", "clusters", "collapsed_faces", "duplicate_faces")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name.startswith("ico"):
        return R.icosphere(int(name[3:]))
    if name == "extra":                                  # vertices no face names, inside and outside the sphere's cells
        v, f = R.icosphere(3)
        return np.concatenate([v, np.random.default_rng(3).random((40, 3)) * 4 - 2]), f
    return {"cube": R.cube, "patch": R.two_layer_patch, "slab": R.slab}[name]()


def device_run(v, f, c, **kw):
    out = ops.mesh_simplify(cuda(v), cuda(f), None if c is None else cuda(c), **kw)
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}


def same(got, want):
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, k
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in NUMBERS:
        assert got[k] == want[k], (k, got[k], want[k])


def check(v, f, c, **kw):
    want = R.simplify(v, f, c, **kw)
    got = device_run(v, f, c, **kw)
    same(got, want)
    same(device_run(v, f, c, **kw), got)                 # a rerun gives the same bits
    return got


@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("name,cell", [("ico4", 0.1), ("ico4", 0.25), ("ico5", 0.05), ("ico5", 0.13)])
def test_icosphere_bit_for_bit(name, cell, placement, with_colors):
    v, f = mesh(name)
    assert (len(v), len(f)) == {"ico4": (2562, 5120), "ico5": (10242, 20480)}[name]
    got = check(v, f, R.colors_of(len(v)) if with_colors else None, cell=cell, placement=placement)
    assert 0 < len(got["verts"]) < len(v) and (placement == "mean") == (not got["placed"].any())


@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("name,cell", [("cube", 0.3), ("patch", 0.25), ("slab", 0.25), ("extra", 0.3)])
def test_fixtures_bit_for_bit(name, cell, placement):
    v, f = mesh(name)
    got = check(v, f, R.colors_of(len(v)), cell=cell, placement=placement)
    if name == "patch":
        assert got["duplicate_faces"] > 0 and (got["face_map"] < len(f) // 2).all()
    if name == "slab":
        assert len(got["faces"]) == 2 * len(np.unique(np.sort(got["faces"], 1), axis=0))
    if name == "extra":
        assert (got["vertex_map"][-40:] == -1).any() and len(got["faces"]) > 0


@pytest.mark.parametrize("V,F", [(n, n) for n in (1, 63, 64, 65, 255, 256, 257)] + [(257, 1), (3, 257), (64, 256), (1024, 86)])
def test_counts_around_a_wave_and_a_block(V, F):
    v, f = R.soup(V, F, seed=V + F)
    check(v, f, R.colors_of(V), cell=0.25)
    check(v, f, None, cell=0.05, placement="mean")       # nearly every vertex a cluster of its own


def test_one_cell_gives_an_empty_mesh():
    v, f = mesh("ico3")
    assert len(f) > ops.SIMPLIFY_BLOCK                   # the one quadric run is longer than a block
    got = check(v, f, R.colors_of(len(v)), cell=10.0)
    assert len(got["verts"]) == 0 and len(got["faces"]) == 0 and (got["vertex_map"] == -1).all()
    assert got["clusters"] == 1 and got["collapsed_faces"] == len(f) and got["colors"].shape == (0, 3)


def test_no_faces_and_no_vertices():
    v, _ = mesh("ico3")
    none = np.zeros((0, 3), np.int32)
    got = check(v, none, R.colors_of(len(v)), cell=0.3)
    assert len(got["verts"]) == 0 and got["vertex_map"].shape == (len(v),)
    check(np.zeros((0, 3)), none, None, cell=0.3)


@pytest.mark.parametrize("N", [1, 300, 2000])
def test_target_mode(N):
    v, f = mesh("ico4")
    want = R.simplify(v, f, None, target_vertices=N)
    got = device_run(v, f, None, target_vertices=N)
    assert got["cell"] == want["cell"] and got["cell"] > 0.0
    assert len(got["verts"]) <= N and ops.simplify_count_cells(cuda(v), got["cell"]) <= N
    same(got, want)
    small = device_run(v, f, R.colors_of(len(v)), target_vertices=len(v))
    same(small, R.simplify(v, f, R.colors_of(len(v)), target_vertices=len(v)))
    assert small["cell"] == 0.0 and np.array_equal(small["verts"], v)


def test_argument_errors_launch_nothing():
    v, f = mesh("ico3")
    tv, tf, tc = cuda(v), cuda(f), cuda(R.colors_of(len(v)))

    def bad(**kw):
        a = dict(verts=tv, faces=tf, colors=tc, cell=0.3)
        a.update(kw)
        with pytest.raises(UfrError):
            ops.mesh_simplify(**a)

    vn, vi = tv.clone(), tv.clone()
    vn[17, 1], vi[5, 2] = float("nan"), float("inf")
    fh, fl = tf.clone(), tf.clone()
    fh[3, 1], fl[0, 0] = len(v), -1
    ops.profile_enable(True)                             # every launch of the library is recorded from here on
    bad(verts=vn)
    bad(verts=vi)
    bad(faces=fh)
    bad(faces=fl)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        bad(cell=cell)
    bad(cell=None)                                       # neither size
    bad(target_vertices=10)                              # both
    bad(cell=None, target_vertices=0)
    bad(cell=1e-7)                                       # more than 2^21 - 4 cells on an axis
    bad(placement="median")
    bad(verts=tv.float())
    bad(faces=tf.long())
    bad(colors=tc.float())
    bad(colors=tc[:-1])
    bad(verts=tv[:, :2].contiguous())
    bad(faces=tf[:, :2].contiguous())
    bad(verts=tv.cpu())
    # the library itself refuses what ops refuses: straight through ctypes
    import ctypes as C

    lib = _lib.load()
    p, n = tv.data_ptr(), 1 << 16
    o = (C.c_double * 3)(0.0, 0.0, 0.0)
    t = C.c_int64(0)
    assert lib.ufr_simplify_workspace_bytes(0) == 0 and lib.ufr_simplify_workspace_bytes(2 ** 31) == 0
    assert lib.ufr_simplify_clusters(p, p, 0, p, p, 1, p, n, C.byref(t), None) != 0
    assert lib.ufr_simplify_clusters(p, p, 4, p, p, 4, p, 8, C.byref(t), None) != 0 and b"workspace" in lib.ufr_last_error()
    assert lib.ufr_simplify_clusters(p, None, 4, p, p, 4, p, n, C.byref(t), None) != 0
    assert lib.ufr_simplify_face_keys(p, p, 4, 0, p, None) != 0
    assert lib.ufr_simplify_face_keys(p, p, 2 ** 31, 4, p, None) != 0
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ufr_simplify_quadrics(p, p, p, 4, 4, 2, o, cell, p, p, p, None) != 0
        assert lib.ufr_simplify_place(p, p, p, p, 2, o, cell, 0, p, p, None) != 0
    assert lib.ufr_simplify_quadrics(p, p, p, 4, 4, 5, o, 1.0, p, p, p, None) != 0          # more clusters than vertices
    assert lib.ufr_simplify_place(p, p, p, p, 2, o, 1.0, 2, p, p, None) != 0 and b"placement" in lib.ufr_last_error()
    assert lib.ufr_simplify_face_triples(p, p, 4, 4, None, p, p, None) != 0
    assert lib.ufr_simplify_face_heads(p, p, p, 0, p, None) != 0
    assert lib.ufr_simplify_compact_faces(p, p, 4, 2, p, p, -1, p, p, n, C.byref(t), None) != 0
    assert lib.ufr_simplify_compact_faces(p, p, 4, 2, None, p, 4, p, p, n, C.byref(t), None) != 0
    assert lib.ufr_simplify_compact_vertices(p, 2, p, None, p, p, p, 4, None, 3, p, None, p, p, 2, p, p, p, n, C.byref(t), None) != 0
    assert lib.ufr_simplify_compact_vertices(p, 2, p, p, p, p, p, 4, p, 3, p, None, p, p, 2, p, p, p, n, C.byref(t), None) != 0
    launched = ops.profile_read()
    ops.profile_enable(False)
    assert launched == {}, launched


def test_command_end_to_end(tmp_path, capsys):
    mesh_dir, out_dir = str(tmp_path / "mesh"), str(tmp_path / "simple")
    os.makedirs(mesh_dir)
    v, f = mesh("ico4")
    colors = R.colors_of(len(v))
    CMesh.write_ply(os.path.join(mesh_dir, "scan7.ply"), v, f, colors)
    CM.write_ply(os.path.join(mesh_dir, "scan9.ply"), v, f)
    assert SM.main(["--mesh_dir", mesh_dir, "--out_dir", out_dir, "--scans", "7", "9", "--ratio", "0.1"]) == 0
    out = capsys.readouterr().out
    report = json.load(open(os.path.join(out_dir, "simplify_mesh.json")))
    assert sorted(report) == ["scan7", "scan9"]
    v32 = v.astype(np.float32).astype(np.float64)        # what the PLY holds
    want = R.simplify(v32, f, colors, target_vertices=257)
    for name, has_colors in (("scan7", True), ("scan9", False)):
        ov, of, oc = dtu_eval.read_ply(os.path.join(out_dir, name + ".ply"), with_colors=True)
        r = report[name]
        assert (r["vertices_in"], r["faces_in"], r["vertices_out"], r["faces_out"]) == (len(v), len(f), len(ov), len(of))
        assert 0 < len(ov) <= 257 and r["cell"] == want["cell"] and r["colors"] == has_colors
        assert np.array_equal(ov, want["verts"].astype(np.float32).astype(np.float64)) and np.array_equal(of, want["faces"])
        assert (oc is not None) == has_colors and (oc is None or np.array_equal(oc, want["colors"]))
        assert r["quadric_share"] == float(want["placed"].mean()) and r["collapsed_faces"] == want["collapsed_faces"]
        assert r["duplicate_faces"] == want["duplicate_faces"] and r["placement"] == "quadric"
        assert "%s: %d -> %d vertices" % (name, len(v), len(ov)) in out
        # the output goes on as it stands: the rasteriser takes it
        K = CR.intrinsics(24, 32, 30.0)
        c2w = CR.ring_cameras(1, 3.0)[:1]
        frames = ops.raster_frames(cuda(ov), cuda(of), np.linalg.inv(K / K[2, 2]), np.stack(c2w), 24, 32,
                                   colors=None if oc is None else cuda(oc), return_face_ids=True)
        assert (frames["face_id"].cpu().numpy() >= 0).any()
    # --ply and --cell, mean placement
    assert SM.main(["--out_dir", out_dir, "--ply", os.path.join(mesh_dir, "scan9.ply"), "--cell", "0.2", "--placement", "mean"]) == 0
    ov, of = dtu_eval.read_ply(os.path.join(out_dir, "scan9.ply"))
    want = R.simplify(v32, f, None, cell=0.2, placement="mean")
    assert np.array_equal(ov, want["verts"].astype(np.float32).astype(np.float64)) and np.array_equal(of, want["faces"])
