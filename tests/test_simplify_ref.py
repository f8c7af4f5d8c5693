"""Mesh simplification (uforecon_amd/simplify_mesh.py, csrc/mesh_simplify.hip), the parts that need no GPU: known answers and
invariants on the numpy statement (simplify_ref.py), the header section against the ctypes signatures and the command line's
parser.  The fixtures built here are what test_gpu_simplify_mesh.py runs on the device against the same statement."""
import os
import re

import numpy as np
import pytest

import simplify_ref as R
from uforecon_amd import _lib, ops, simplify_mesh as SM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def rotated_triples(faces):
    first = np.argmin(faces, 1)
    return np.stack([faces[np.arange(len(faces)), (first + e) % 3] for e in range(3)], 1)


def check_invariants(v, f, colors, r, cell):
    """what holds for every output of the rule"""
    V, F = len(v), len(f)
    ov, of = r["verts"], r["faces"]
    Vo, Fo = len(ov), len(of)
    assert ov.dtype == np.float64 and of.dtype == np.int32 and r["placed"].dtype == np.uint8 and r["count"].dtype == np.int32
    assert r["vertex_map"].shape == (V,) and r["face_map"].shape == (Fo,) and r["placed"].shape == (Vo,) and r["count"].shape == (Vo,)
    # every output vertex lies within cell / 2 of its cell centre on each axis
    assert (np.abs(ov - r["centres"]) <= cell / 2).all()
    # no face has a repeated corner, no two faces share a rotated triple, every output vertex is referenced
    assert Fo == 0 or ((of[:, 0] != of[:, 1]) & (of[:, 1] != of[:, 2]) & (of[:, 0] != of[:, 2])).all()
    assert len(np.unique(rotated_triples(of), axis=0)) == Fo
    assert (of[:, 0] <= of.min(1)).all()                                  # the smallest number stands first
    assert np.array_equal(np.unique(of), np.arange(Vo))
    # the maps agree with the outputs
    vm, fm = r["vertex_map"], r["face_map"]
    assert ((vm >= -1) & (vm < Vo)).all() and (np.diff(fm) > 0).all() and ((fm >= 0) & (fm < F)).all()
    assert np.array_equal(rotated_triples(vm[f[fm]]), of)
    assert np.array_equal(np.bincount(vm[vm >= 0], minlength=Vo), r["count"])
    dropped = np.setdiff1d(np.arange(F), fm)
    mapped = vm[f[dropped]]
    collapsed = (mapped[:, 0] == mapped[:, 1]) | (mapped[:, 1] == mapped[:, 2]) | (mapped[:, 0] == mapped[:, 2]) | (mapped < 0).any(1)
    assert collapsed.sum() + r["duplicate_faces"] == len(dropped)
    if (~collapsed).any():                                                # a dropped duplicate has a survivor with a lower index
        kept = {tuple(t): i for t, i in zip(rotated_triples(vm[f[fm]]).tolist(), fm.tolist())}
        for i, t in zip(dropped[~collapsed].tolist(), rotated_triples(mapped[~collapsed]).tolist()):
            assert kept[tuple(t)] < i
    # colours follow the integer rounding rule
    if colors is not None:
        for o in range(0, Vo, max(1, Vo // 50)):
            members = np.flatnonzero(vm == o)
            s, c = colors[members].astype(np.int64).sum(0), len(members)
            assert np.array_equal(r["colors"][o], (2 * s + c) // (2 * c))
    else:
        assert r["colors"] is None


# ------------------------------------------------------------------ the cube
def test_cube_corners_are_kept_by_the_quadric_and_lost_by_the_mean():
    v, f = R.cube(9)
    assert len(v) == 6 * 81 - 12 * 9 + 8 and len(f) == 6 * 64 * 2
    cell = 0.3
    q = R.simplify(v, f, cell=cell)
    m = R.simplify(v, f, cell=cell, placement="mean")
    # x_k - corner_k = w (xb_k - corner_k) / (a_k + w) with trace / a_k = 3 by the cube's symmetry and |xb_k - corner_k| <= cell / 2
    bound = 3 * 2.0 ** -10 * (cell / 2)
    for corner in np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64):
        dq = np.abs(q["verts"] - corner).max(1)
        assert dq.min() <= bound, (corner, dq.min())
        assert q["placed"][np.argmin(dq)] == 1
        assert np.linalg.norm(m["verts"] - corner, axis=1).min() > 0.05
    assert q["placed"].mean() > 0.5 and not m["placed"].any()         # flat cells: x = the mean up to rounding, either may win


@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("mesh,cell", [("cube", 0.3), ("ico4", 0.1), ("ico4", 0.25)])
def test_invariants(mesh, cell, placement):
    v, f = R.cube(9) if mesh == "cube" else R.icosphere(4)
    if mesh == "ico4":
        assert len(v) == 2562 and len(f) == 5120
    colors = R.colors_of(len(v))
    r = R.simplify(v, f, colors, cell=cell, placement=placement)
    assert 0 < len(r["verts"]) < len(v) and 0 < len(r["faces"]) < len(f)
    check_invariants(v, f, colors, r, cell)
    r2 = R.simplify(v, f, None, cell=cell, placement=placement)
    check_invariants(v, f, None, r2, cell)
    assert np.array_equal(r2["verts"], r["verts"]) and np.array_equal(r2["faces"], r["faces"])


def test_sphere_quadric_is_taken_in_most_cells():
    v, f = R.icosphere(4)
    r = R.simplify(v, f, cell=0.1)
    assert r["placed"].mean() > 0.7
    assert np.abs(np.linalg.norm(r["verts"], axis=1) - 1.0).max() < 0.1 * 3 ** 0.5


# ------------------------------------------------------------------ duplicates and opposite pairs
def test_two_layer_patch_keeps_the_lowest_input_index():
    cell = 0.25
    v, f = R.two_layer_patch(13, cell)
    r = R.simplify(v, f, cell=cell)
    assert r["duplicate_faces"] > 0
    check_invariants(v, f, None, r, cell)
    half = len(f) // 2
    vm = r["vertex_map"]
    t0, t1 = rotated_triples(vm[f[:half]]), rotated_triples(vm[f[half:]])
    assert np.array_equal(t0, t1)                                         # the copy's faces fall on the same triples
    assert (r["face_map"] < half).all()                                   # so none of them survives


def test_slab_keeps_both_faces_of_an_opposite_pair():
    cell = 0.25
    v, f = R.slab(13, 0.02)
    r = R.simplify(v, f, cell=cell)
    check_invariants(v, f, None, r, cell)
    of = r["faces"]
    have = {tuple(t) for t in rotated_triples(of).tolist()}
    mirrored = rotated_triples(of[:, ::-1].copy())
    assert len(of) > 0 and all(tuple(t) in have for t in mirrored.tolist())
    assert len(of) == 2 * len(np.unique(np.sort(of, 1), axis=0))


def test_unreferenced_vertices_and_one_cell():
    v, f = R.icosphere(3)
    extra = np.random.default_rng(3).random((40, 3)) * 4 - 2
    r = R.simplify(np.concatenate([v, extra]), f, cell=0.3)
    check_invariants(np.concatenate([v, extra]), f, None, r, 0.3)
    base = R.simplify(v, f, cell=0.3)
    assert len(r["faces"]) > 0 and (r["vertex_map"][len(v):] == -1).sum() > 0
    one = R.simplify(v, f, cell=10.0)
    assert len(one["verts"]) == 0 and len(one["faces"]) == 0 and (one["vertex_map"] == -1).all() and one["clusters"] == 1
    assert one["collapsed_faces"] == len(f) and len(base["verts"]) > 0
    none = R.simplify(v, np.zeros((0, 3), np.int32), cell=0.3)
    assert len(none["verts"]) == 0 and len(none["faces"]) == 0 and (none["vertex_map"] == -1).all()


# ------------------------------------------------------------------ target size
@pytest.mark.parametrize("N", [1, 100, 500])
def test_target_mode_stays_under_the_target(N):
    v, f = R.icosphere(3)
    r = R.simplify(v, f, target_vertices=N)
    assert len(r["verts"]) <= N and r["cell"] > 0 and R.count_cells(v, r["cell"]) <= N
    if N > 1:
        assert len(r["verts"]) > N // 4                                   # and not absurdly far under it
    check_invariants(v, f, None, r, r["cell"])


def test_target_mode_returns_a_small_mesh_unchanged():
    v, f = R.icosphere(1)
    c = R.colors_of(len(v))
    for N in (len(v), len(v) + 5):
        r = R.simplify(v, f, c, target_vertices=N)
        assert r["cell"] == 0.0 and np.array_equal(r["verts"], v) and np.array_equal(r["faces"], f) and np.array_equal(r["colors"], c)
        assert np.array_equal(r["vertex_map"], np.arange(len(v))) and np.array_equal(r["face_map"], np.arange(len(f)))


# ------------------------------------------------------------------ header, signatures, command line
def test_header_section_and_signatures():
    import ctypes as C

    from uforecon_amd.build import SOURCES

    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert text.count("/* ---- mesh simplification (ABI 507, additive) ----") == 1
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    assert text.index("/* ---- mesh colouring (ABI 507, additive)") < text.index("/* ---- mesh simplification (ABI 507, additive)")
    section = text[text.index("mesh simplification (ABI 507, additive)"):]
    section = section[:section.index("/* ----", 10)]
    assert "point-cloud filtering" in text[text.index(section) + len(section):][:60]      # directly before the next heading
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
    assert len(found) == 9 and all(n.startswith("ufr_simplify_") for n in found)
    assert sorted(found) == sorted(n for n in _lib.SIGNATURES if n.startswith("ufr_simplify_"))
    assert "#define UFR_SIMPLIFY_QUADRIC 0" in code and "#define UFR_SIMPLIFY_MEAN 1" in code
    assert ops.SIMPLIFY_PLACEMENTS == {"quadric": 0, "mean": 1}
    for phrase in ("Open3D was not compared", "no edge-collapse decimation", "no topology guarantee", "normals are not carried"):
        assert phrase in " ".join(section.replace(" * ", " ").split()), phrase
    assert "mesh_simplify.hip" in SOURCES
    internal = open(os.path.join(ROOT, "uforecon_amd", "csrc", "ufr_internal.h")).read()
    assert re.search(r"constexpr int kSimplifyThreads = (\d+);", internal).group(1) == str(ops.SIMPLIFY_BLOCK)
    assert ops.SIMPLIFY_MAX_CELLS == R.MAX_CELLS and ops.SIMPLIFY_BISECTION_STEPS == R.BISECTION_STEPS


def test_parser_wants_exactly_one_size():
    p = SM.make_parser()
    for bad in (["--cell", "0.1", "--target_vertices", "10"], ["--cell", "0.1", "--ratio", "0.5"],
                ["--target_vertices", "10", "--ratio", "0.5"], []):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    a = p.parse_args(["--ratio", "0.1"])
    assert (a.cell, a.target_vertices, a.ratio, a.placement) == (None, None, 0.1, "quadric")
    assert (a.mesh_dir, a.out_dir) == ("./outputs/mesh/final", "./outputs/mesh/simple")
    assert p.parse_args(["--cell", "2", "--placement", "mean"]).placement == "mean"
    with pytest.raises(SystemExit):
        SM.main(["--cell", "-1"])
    with pytest.raises(SystemExit):
        SM.main(["--ratio", "1.5"])


def test_command_reports_missing_and_faceless_meshes(tmp_path, capsys):
    from uforecon_amd import clean_mesh as CM

    mesh_dir, out_dir = str(tmp_path / "mesh"), str(tmp_path / "out")
    os.makedirs(mesh_dir)
    v, _ = R.icosphere(0)
    CM.write_ply(os.path.join(mesh_dir, "scan4.ply"), v, np.zeros((0, 3), np.int32))
    assert SM.main(["--mesh_dir", mesh_dir, "--out_dir", out_dir, "--scans", "4", "9", "--cell", "0.5"]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("scan4: ") and lines[0].endswith("has no faces")
    assert lines[1].startswith("scan9: no mesh at ")
    import json
    assert json.load(open(os.path.join(out_dir, "simplify_mesh.json"))) == {}
