"""Point-cloud filtering (uforecon_amd/pcd_filter.py, csrc/points_filter.hip), the parts that need no GPU: the numpy restatement
(pcd_ref.py) against scipy's k-d tree and against a loop in python floats, the statistical rule on a cloud with known outliers,
the header section against the ctypes signatures, the command line's flags and defaults, and the PLY writer against the reader."""
import math
import os
import re

import numpy as np
import pytest

import pcd_ref as R
from uforecon_amd import _lib, dtu_eval, pcd_filter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CLOUD = R.sphere_cloud()          # 2000 points on the unit sphere (radial noise 0.002) + 12 at radius > 1.6
N_SURFACE = 2000


# ------------------------------------------------------------------ pcd_ref.knn
@pytest.mark.parametrize("k", [16, 30])
def test_knn_ref_equals_scipy_kdtree(k):
    from scipy.spatial import cKDTree

    idx, dist = R.knn(CLOUD, CLOUD, k)
    d, i = cKDTree(CLOUD).query(CLOUD, k)
    assert np.array_equal(dist.view(np.int64), d.view(np.int64))          # the same bits
    distinct = np.ones_like(dist, bool)                       # slots whose distance no neighbouring slot shares
    distinct[:, 1:] &= dist[:, 1:] != dist[:, :-1]
    distinct[:, :-1] &= dist[:, 1:] != dist[:, :-1]
    assert distinct.mean() > 0.99
    assert np.array_equal(idx[distinct], i[distinct].astype(np.int32))


def _loop_knn(query, ref, k, max_dist=math.inf, exclude_self=False):
    """the rule text of include/ufr.h read literally, in python floats"""
    idx, dist = [], []
    for qi, q in enumerate(query):
        cand = []
        if all(math.isfinite(float(v)) for v in q):
            for ri, r in enumerate(ref):
                if exclude_self and ri == qi:
                    continue
                dx, dy, dz = float(q[0]) - float(r[0]), float(q[1]) - float(r[1]), float(q[2]) - float(r[2])
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 <= max_dist * max_dist:
                    cand.append((d2, ri))
        cand = sorted(cand)[:k]
        idx.append([c[1] for c in cand] + [-1] * (k - len(cand)))
        dist.append([math.sqrt(c[0]) for c in cand] + [math.inf] * (k - len(cand)))
    return np.array(idx, np.int32).reshape(len(query), k), np.array(dist, np.float64).reshape(len(query), k)


def _small_cloud():
    lattice = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3)       # 27 points, many equal distances
    rng = np.random.default_rng(5)
    extra = rng.uniform(0, 2, (12, 3))
    return np.concatenate([lattice, extra, extra[:1]])                                               # 40 points, one exact duplicate


@pytest.mark.parametrize("k,max_dist,exclude_self", [(5, math.inf, False), (8, math.inf, True), (32, math.inf, False),
                                                     (6, 1.0, True), (7, 1.5, False)])
def test_knn_ref_equals_a_python_loop(k, max_dist, exclude_self):
    pts = _small_cloud()
    assert len(pts) == 40
    got_i, got_d = R.knn(pts, pts, k, max_dist, exclude_self)
    want_i, want_d = _loop_knn(pts, pts, k, max_dist, exclude_self)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_d.view(np.int64), want_d.view(np.int64))


def test_knn_ref_k_above_nr_and_a_query_that_is_not_finite():
    pts = _small_cloud()
    q = pts[:6].copy()
    q[2, 1] = np.nan
    got_i, got_d = R.knn(q, pts[:4], 9)
    want_i, want_d = _loop_knn(q, pts[:4], 9)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d.view(np.int64), want_d.view(np.int64))
    assert (got_i[2] == -1).all() and np.isinf(got_d[2]).all()
    assert (got_i[0, 4:] == -1).all() and (got_i[0, :4] >= 0).all()


# ------------------------------------------------------------------ the statistical rule
@pytest.mark.parametrize("nb", [8, 20])
def test_statistical_rule_removes_exactly_the_far_points(nb):
    keep, avg, thr = R.statistical(CLOUD, nb, 2.0)
    assert keep[:N_SURFACE].all() and not keep[N_SURFACE:].any()
    ratio = avg / thr
    # well away from 1 on both sides (0.71 / 2.83 at 8 neighbours, 0.75 / 2.44 at 20), where rounding moves a ratio by about
    # 1e-13: the mask does not depend on how the sums round
    assert ratio[:N_SURFACE].max() < 0.9 and ratio[N_SURFACE:].min() > 1.1


def test_radius_rule_counts_inclusively():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float64)
    assert R.radius(pts, 2, 1.0).tolist() == [True, False, False, False]
    assert R.radius(pts, 1, 1.0).tolist() == [True, True, True, False]


# ------------------------------------------------------------------ normals and voxels of the restatement
def test_normals_ref_on_a_plane_and_with_too_few_neighbours():
    rng = np.random.default_rng(1)
    pts = np.concatenate([np.c_[rng.uniform(-1, 1, (50, 2)), np.zeros(50)], [[9.0, 9.0, 9.0]]])
    idx, _ = R.knn(pts, pts, 6, max_dist=1.0)
    n, curv, valid, _ = R.normals(pts, idx)
    assert valid[:50].all() and valid[50] == 0 and (n[50] == 0).all() and curv[50] == 0
    assert np.allclose(n[:50], [0, 0, 1], atol=1e-12) and np.allclose(curv[:50], 0, atol=1e-12)
    n2, _, _, (_, _, best) = R.normals(pts, idx, np.array([[0.0, 0.0, -4.0]]))
    assert np.allclose(n2[:50], [0, 0, -1], atol=1e-12) and best[:50].min() > 0.9


def test_voxel_ref_means_counts_and_half_way_colours():
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.3, 0.1, 0.1], [0.3, 0.3, 0.3]], np.float64)
    col = np.array([[1, 10, 0], [2, 11, 0], [200, 0, 0], [4, 13, 255]], np.uint8)
    p, c, n, count = R.voxel_mean(pts, 1.0, col)
    assert n is None and count.tolist() == [3, 1]
    assert np.array_equal(p[0], ((pts[0] + pts[1]) + pts[3]) / 3.0) and np.array_equal(p[1], pts[2])
    assert c.tolist() == [[2, 11, 85], [200, 0, 0]]                # 7/3 -> 2, 34/3 -> 11, 255/3 = 85
    _, c2, _, _ = R.voxel_mean(pts[:2], 1.0, col[:2])
    assert c2.tolist() == [[2, 11, 0]]                             # 1.5 and 10.5: halves go up
    with pytest.raises(ValueError):
        R.voxel_mean(np.array([[0.0, 0, 0], [1.0, 0, 0]]), 1e-7)


# ------------------------------------------------------------------ header, signatures
NEW_SYMBOLS = {"ufr_points_knn": 14, "ufr_points_normals": 10, "ufr_points_voxel_mean_workspace_bytes": 1, "ufr_points_voxel_mean": 14}


def test_header_section_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert hdr.count("/* ---- point-cloud filtering (ABI 507, additive) ----") == 1
    section = hdr[hdr.index("point-cloud filtering (ABI 507, additive)"):]
    end = section.find("/* ----", 10)
    section = section[:end if end > 0 else len(section)]
    code = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    found = {}
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code):
        found[name] = len(params.split(","))
        assert _lib.SIGNATURES[name][0] is (_lib.C.c_int if res == "int" else _lib.C.c_size_t)
    assert found == NEW_SYMBOLS
    for name, n_args in NEW_SYMBOLS.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert "#define UFR_KNN_MAX_K 32" in code and pcd_filter.KNN_MAX_K == 32 == R.KNN_MAX_K
    assert _lib.ABI_VERSION == 507 and "#define UFR_ABI_VERSION 507" in hdr
    assert "neither library was compared" in section


# ------------------------------------------------------------------ the command line
def test_parser_flags_and_defaults():
    args = pcd_filter.make_parser().parse_args(["--out_dir", "x"])
    assert vars(args) == dict(root_dir="./outputs", out_dir="x", scans=None, ply=None, voxel_size=0.0, nb_neighbors=20, std_ratio=2.0,
                              radius=0.0, nb_points=0, normals=0, dataset_dir=None, views=[23, 24, 33])
    args = pcd_filter.make_parser().parse_args("--root_dir a --out_dir b --scans 24 37 --voxel_size 0.5 --nb_neighbors 8 --std_ratio 1.5 "
                                               "--radius 2 --nb_points 4 --normals 30 --dataset_dir d --views 1 2 --ply p.ply q.ply".split())
    assert (args.scans, args.ply, args.voxel_size, args.nb_neighbors, args.std_ratio) == ([24, 37], ["p.ply", "q.ply"], 0.5, 8, 1.5)
    assert (args.radius, args.nb_points, args.normals, args.dataset_dir, args.views) == (2.0, 4, 30, "d", [1, 2])


def test_out_dir_equal_to_root_dir_is_refused(tmp_path, capsys):
    os.makedirs(tmp_path / "pcd")
    assert pcd_filter.main(["--root_dir", str(tmp_path), "--out_dir", str(tmp_path / "pcd" / "..")]) == 2
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and "overwrite" in out[0]
    assert not os.path.exists(tmp_path / "pcd_filter.json")
    assert pcd_filter.main(["--root_dir", str(tmp_path), "--out_dir", str(tmp_path / "f"), "--normals", "33"]) == 2
    assert pcd_filter.main(["--root_dir", str(tmp_path), "--out_dir", str(tmp_path / "f"), "--normals", "2"]) == 2
    assert "at least 3" in capsys.readouterr().out


def test_a_scan_without_a_file_is_reported_and_skipped(tmp_path, capsys):
    assert pcd_filter.main(["--root_dir", str(tmp_path), "--out_dir", str(tmp_path / "f"), "--scans", "24"]) == 0
    assert "cloud not found" in capsys.readouterr().out
    import json

    assert json.load(open(tmp_path / "f" / "pcd_filter.json"))["scans"] == {}


# ------------------------------------------------------------------ files
def test_ply_round_trip_with_normals(tmp_path):
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    nrm = rng.standard_normal((37, 3)).astype(np.float32)
    path = str(tmp_path / "c.ply")
    pcd_filter.write_ply(path, xyz, rgb, nrm)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header")].decode()
    assert "format binary_little_endian 1.0" in header
    assert re.findall(r"property (\w+) (\w+)", header) == [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"),
                                                             ("uchar", "green"), ("uchar", "blue"), ("float", "nx"), ("float", "ny"),
                                                             ("float", "nz")]
    v, f, c = dtu_eval.read_ply(path, with_colors=True)
    assert f is None and np.array_equal(v, xyz.astype(np.float64)) and np.array_equal(c, rgb)
    pcd_filter.write_ply(path, xyz)                                  # positions only
    v, f, c = dtu_eval.read_ply(path, with_colors=True)
    assert c is None and np.array_equal(v, xyz.astype(np.float64))
    assert len(open(path, "rb").read()) == open(path, "rb").read().index(b"end_header\n") + 11 + 37 * 12


def test_camera_centres(tmp_path):
    os.makedirs(tmp_path / "cameras")
    E = np.eye(4)
    E[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    E[:3, 3] = [1, 2, 3]
    with open(tmp_path / "cameras" / "00000023_cam.txt", "w") as f:
        f.write("extrinsic\n" + "\n".join(" ".join(str(v) for v in row) for row in E) + "\n\nintrinsic\n1 0 0\n0 1 0\n0 0 1\n\n425 2.5\n")
    c = pcd_filter.camera_centres(str(tmp_path), [23])
    assert c.shape == (1, 3) and np.allclose(E[:3, :3] @ c[0] + E[:3, 3], 0)
