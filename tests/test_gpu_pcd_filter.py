"""Point-cloud filtering on the GPU (csrc/points_filter.hip through uforecon_amd/ops.py and uforecon_amd/pcd_filter.py) against
the numpy restatement pcd_ref.py on the same inputs: neighbour indices, distances, masks, means and voxel outputs bit for bit,
the threshold and the eigenvectors within bounds that are derived where they are used."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import pcd_ref as R
from uforecon_amd import depth_fusion, dtu_eval, ops, pcd_filter
from uforecon_amd import render_trajectory as RT
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

CLOUD = R.sphere_cloud()          # 2000 points on the unit sphere (radial noise 0.002) + 12 at radius > 1.6
N_SURFACE = 2000


def _cuda(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _ref_knn_cloud(k, exclude_self):
    return R.knn(CLOUD, CLOUD, k, exclude_self=exclude_self)


def _check_knn(query, ref, k, max_dist=np.inf, exclude_self=False, want=None):
    r = _cuda(ref)
    q = r if exclude_self or query is ref else _cuda(query)
    idx, dist = ops.knn_points(q, r, k, max_dist, exclude_self)
    assert idx.shape == (len(query), k) and idx.dtype == torch.int32 and dist.shape == (len(query), k) and dist.dtype == torch.float64
    want_i, want_d = want if want is not None else R.knn(query, ref, k, max_dist, exclude_self)
    assert np.array_equal(idx.cpu().numpy(), want_i)
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_d))
    return idx, dist


# ------------------------------------------------------------------ k nearest neighbours
@pytest.mark.parametrize("nr", [1, 5, 6])
def test_knn_small_reference_sets(nr):
    _check_knn(CLOUD[:50], CLOUD[100:100 + nr], 5)


@pytest.mark.parametrize("k", [1, 2, 20, 32])
def test_knn_list_lengths(k):
    _check_knn(CLOUD[::4], CLOUD, k)


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257])
def test_knn_query_counts_around_the_block_sizes(nq):
    _check_knn(CLOUD[:nq], CLOUD, 7)


def test_knn_duplicates_and_one_cell():
    dup = np.concatenate([CLOUD[:100], CLOUD[:100], CLOUD[:3]])
    _check_knn(dup, dup, 5)
    _check_knn(dup, dup, 5, exclude_self=True)
    one = np.tile(CLOUD[7:8], (40, 1))
    idx, dist = _check_knn(one, one, 8)
    assert (idx.cpu().numpy() == np.arange(8)).all() and (dist == 0).all()


def test_knn_lattice_ties_go_to_the_lower_index():
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    _check_knn(g, g, 20)
    _check_knn(g, g, 32, exclude_self=True)
    _check_knn(g, g, 7, max_dist=1.0)                  # exactly the six neighbours at distance 1 and the point: inclusive
    p = np.random.default_rng(3).permutation(len(g))   # the same lattice in another order: other indices win the ties
    _check_knn(g[p], g[p], 20)


@pytest.mark.parametrize("exclude_self", [False, True])
def test_knn_sphere_cloud(exclude_self):
    _check_knn(CLOUD, CLOUD, 20, exclude_self=exclude_self, want=_ref_knn_cloud(20, exclude_self))


def test_knn_finite_max_dist_leaves_empty_slots():
    idx, dist = _check_knn(CLOUD, CLOUD, 20, max_dist=0.08, exclude_self=True)
    filled = (idx >= 0).sum(1).cpu().numpy()
    assert filled.min() == 0 and 0 < filled.max() <= 20 and len(np.unique(filled)) > 3
    assert bool(torch.isinf(dist[idx < 0]).all()) and bool((dist[idx >= 0] <= 0.08).all())


def test_knn_query_row_that_is_not_finite():
    q = CLOUD[:10].copy()
    q[3, 1] = np.nan
    q[5, 0] = np.inf
    idx, dist = _check_knn(q, CLOUD, 4)
    assert (idx[3] == -1).all() and (idx[5] == -1).all() and bool(torch.isinf(dist[[3, 5]]).all())


def test_knn_k1_equals_nn_distance_below_max_dist():
    rng = np.random.default_rng(11)
    q = _cuda(CLOUD[:700] + 0.05 * rng.standard_normal((700, 3)))
    r = _cuda(CLOUD)
    max_dist = 0.06
    idx, dist = ops.knn_points(q, r, 1, max_dist)
    want = ops.nn_distance(q, r, max_dist)
    below = want < max_dist
    assert 100 < int(below.sum()) < 700
    assert torch.equal(dist[:, 0][below].view(torch.int64), want[below].view(torch.int64))
    assert bool((idx[:, 0][below] >= 0).all()) and bool((idx[:, 0][~below] == -1).all())


def test_knn_two_runs_give_the_same_bits():
    p = _cuda(CLOUD)
    a = ops.knn_points(p, p, 30)
    b = ops.knn_points(p, p, 30)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_knn_argument_errors():
    p = _cuda(CLOUD[:20])
    for bad in (lambda: ops.knn_points(p, p, 0), lambda: ops.knn_points(p, p, 33), lambda: ops.knn_points(p, p, 3, max_dist=0.0),
                lambda: ops.knn_points(p, p.clone(), 3, exclude_self=True), lambda: ops.knn_points(p, p[:0], 3),
                lambda: ops.knn_points(p.cpu(), p.cpu(), 3), lambda: ops.knn_points(p.float(), p, 3)):
        with pytest.raises(UfrError):
            bad()
    nan = p.clone()
    nan[4, 2] = float("nan")
    with pytest.raises(UfrError):
        ops.knn_points(p, nan, 3)
    idx, dist = ops.knn_points(p[:0], p, 3)
    assert idx.shape == (0, 3) and dist.shape == (0, 3)


# ------------------------------------------------------------------ outlier filters
@pytest.mark.parametrize("nb", [8, 20])
def test_statistical_filter(nb):
    keep, avg, thr = pcd_filter.remove_statistical_outliers(_cuda(CLOUD), nb, 2.0)
    want_keep, want_avg, want_thr = R.statistical(CLOUD, nb, 2.0)
    assert np.array_equal(keep.cpu().numpy(), want_keep)
    assert keep[:N_SURFACE].all() and not keep[N_SURFACE:].any()
    assert np.array_equal(_bits(avg.cpu().numpy()), _bits(want_avg))
    # the order of summation over <= 2^11 positive doubles moves the mean by about N 2^-53 = 2e-13: 1e-10 leaves about 500x
    print("threshold", thr, want_thr, abs(thr - want_thr) / want_thr)
    assert abs(thr - want_thr) <= 1e-10 * want_thr


def test_statistical_filter_point_without_neighbours():
    keep, avg, thr = pcd_filter.remove_statistical_outliers(_cuda(CLOUD[:1]), 8, 2.0)
    want_keep, want_avg, want_thr = R.statistical(CLOUD[:1], 8, 2.0)
    assert bool(torch.isinf(avg).all()) and np.isinf(want_avg).all() and thr == want_thr == float("inf")
    assert keep.tolist() == want_keep.tolist() == [True]            # inf <= inf: the rule as stated keeps it


def test_radius_filter():
    keep = pcd_filter.remove_radius_outliers(_cuda(CLOUD), 4, 0.09)
    want = R.radius(CLOUD, 4, 0.09)
    assert np.array_equal(keep.cpu().numpy(), want)
    assert 0 < want[:N_SURFACE].sum() < N_SURFACE and not want[N_SURFACE:].any()
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)     # distances of exactly 1: inclusive
    keep = pcd_filter.remove_radius_outliers(_cuda(g), 6, 1.0).cpu().numpy()
    assert np.array_equal(keep, R.radius(g, 6, 1.0)) and keep.sum() == 8


# ------------------------------------------------------------------ normals
VIEWS = {"none": None, "one": np.array([[0.0, 0.0, 5.0]]), "two": np.array([[0.0, 0.0, 5.0], [4.0, 0.0, 0.0]])}


@pytest.mark.parametrize("k", [16, 30])
@pytest.mark.parametrize("views", ["none", "one", "two"])
def test_normals(k, views):
    vp = VIEWS[views]
    pts = _cuda(CLOUD)
    idx, _ = ops.knn_points(pts, pts, k)
    idx_h = idx.cpu().numpy()
    n, curv, valid = ops.point_normals(pts, idx, None if vp is None else _cuda(vp))
    n, curv, valid = n.cpu().numpy(), curv.cpu().numpy(), valid.cpu().numpy()
    want_n, want_curv, want_valid, (cov, w, best) = R.normals(CLOUD, idx_h, vp)
    assert np.array_equal(valid, want_valid) and valid.all()
    # the covariance is formed with the kernel's own expressions and order, so it is exact input to both solvers
    length = np.sqrt((n * n).sum(1))
    resid = np.einsum("nij,nj->ni", cov, n) - w[:, :1] * n
    resid = np.sqrt((resid * resid).sum(1)) / np.linalg.norm(cov, axis=(1, 2))
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    dot = (n * want_n).sum(1)
    angle = np.arctan2(np.linalg.norm(np.cross(n, want_n), axis=1), np.abs(dot))
    print("k", k, views, "| len - 1 |", np.abs(length - 1).max(), "residual", resid.max(), "min gap", gap.min(), "max angle", angle.max(),
          "curvature", np.abs(curv - want_curv).max(), "min best cos", None if best is None else best.min())
    assert np.abs(length - 1).max() <= 1e-12
    assert resid.max() <= 1e-12
    # perturbation theory: angle <~ |E| / gap ~ 1e-15 / 1e-3, bound with 1000x margin; at most 1 % may fall under the gap condition
    wide = gap >= 1e-3
    assert wide.all()                                       # on this cloud the reference leaves out none (0.029 at k = 16, 0.059 at 30)
    assert angle[wide].max() <= 1e-9
    assert np.abs(curv - want_curv).max() <= 1e-12          # eigenvalues to a few ulp of |C|, l0 / trace well conditioned
    if vp is not None:
        seen = best >= 1e-6
        assert seen.all()                                   # checked before relying on the 1 % cap: none excluded
        assert (dot[seen] > 0).all()
        towards = ((vp[None] - CLOUD[:, None]) * n[:, None]).sum(2)          # the normal faces at least one viewpoint
        assert (towards.max(1) > 0).all()
    else:
        ax = np.abs(n).argmax(1)                            # the first of equal maxima: ties to the lowest axis
        assert (n[np.arange(len(n)), ax] > 0).all()
        top2 = np.sort(np.abs(want_n), 1)
        clear = top2[:, 2] - top2[:, 1] >= 1e-9             # where the largest component is not a near tie the reference's sign is the same
        assert clear.mean() >= 0.99 and (dot[clear] > 0).all()


def test_normals_with_fewer_than_three_neighbours_are_invalid():
    pts = _cuda(CLOUD[:6])
    idx = torch.full((6, 4), -1, dtype=torch.int32, device="cuda")
    idx[:, 0] = torch.arange(6, dtype=torch.int32)
    idx[1, 1] = 2
    idx[2, 1:] = torch.tensor([3, 4, 5], dtype=torch.int32)
    idx[3, 1:] = torch.tensor([0, 99, -7], dtype=torch.int32)       # an index outside the cloud is an empty slot
    idx[4, 1:] = torch.tensor([-1, 0, 1], dtype=torch.int32)         # empty slots may stand anywhere in the row
    n, curv, valid = ops.point_normals(pts, idx)
    assert valid.tolist() == [0, 0, 1, 0, 1, 0]
    assert bool((n[valid == 0] == 0).all()) and bool((curv[valid == 0] == 0).all())
    want_n, _, want_valid, _ = R.normals(CLOUD[:6], np.where((idx.cpu().numpy() >= 6), -1, idx.cpu().numpy()))
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    assert np.abs(np.abs((n.cpu().numpy() * want_n).sum(1))[[2, 4]] - 1).max() <= 1e-12
    with pytest.raises(UfrError):
        ops.point_normals(pts, idx[:5])
    with pytest.raises(UfrError):
        ops.point_normals(pts, idx.long())


# ------------------------------------------------------------------ voxel mean
def _voxel_box():
    """500 points in a box of 4 x 4 x 4 voxels of edge 1 (grid origin -0.4): one voxel empty, one with a single point, one whose
    two points' colours sum to an odd number."""
    rng = np.random.default_rng(9)
    cells = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    special = {(3, 3, 3): 0, (1, 2, 3): 1, (2, 0, 1): 2}
    rest = [c for c in cells if tuple(c) not in special]
    pick = np.concatenate([np.arange(len(rest)), rng.integers(0, len(rest), 500 - 4 - len(rest))])
    cell = np.concatenate([[(0, 0, 0)], [(1, 2, 3)], [(2, 0, 1)] * 2, np.array(rest)[pick]]).astype(np.float64)
    pts = cell + rng.uniform(0.1, 0.6, (500, 3))
    pts[0] = 0.1                                                  # the minimum corner: the grid origin is 0.1 - 0.5
    col = rng.integers(0, 256, (500, 3)).astype(np.uint8)
    col[2], col[3] = (1, 10, 255), (2, 11, 254)
    nrm = rng.standard_normal((500, 3))
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    order = rng.permutation(500)
    return pts[order], col[order], nrm[order]


def test_voxel_mean():
    pts, col, nrm = _voxel_box()
    want_p, want_c, want_n, want_count = R.voxel_mean(pts, 1.0, col, nrm)
    assert len(want_p) == 63 and (want_count == 1).sum() >= 1 and want_count.sum() == 500
    assert [2, 11, 255] in want_c.tolist()                         # 1.5 -> 2, 10.5 -> 11, 254.5 -> 255
    p, c, n, count = ops.voxel_downsample(_cuda(pts), 1.0, _cuda(col, torch.uint8), _cuda(nrm))
    assert np.array_equal(count.cpu().numpy(), want_count) and count.dtype == torch.int32
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(want_p))
    assert np.array_equal(c.cpu().numpy(), want_c)
    assert np.array_equal(_bits(n.cpu().numpy()), _bits(want_n))
    p2, c2, n2, count2 = ops.voxel_downsample(_cuda(pts), 1.0)
    assert c2 is None and n2 is None and torch.equal(p2, p) and torch.equal(count2, count)
    # more than one block of run heads, voxels of very different sizes
    big = np.concatenate([CLOUD, CLOUD[:700] * 0.999])
    want_p, _, _, want_count = R.voxel_mean(big, 0.05)
    assert len(want_p) > 512
    p, _, _, count = ops.voxel_downsample(_cuda(big), 0.05)
    assert np.array_equal(count.cpu().numpy(), want_count) and np.array_equal(_bits(p.cpu().numpy()), _bits(want_p))


def test_voxel_extent_guard_and_argument_errors():
    two = _cuda(np.array([[0.0, 0, 0], [1.0, 0, 0]]))
    with pytest.raises(UfrError, match="cells"):
        ops.voxel_downsample(two, 1e-7)
    for bad in (lambda: ops.voxel_downsample(two, 0.0), lambda: ops.voxel_downsample(two.cpu(), 1.0),
                lambda: ops.voxel_downsample(two, 1.0, colors=torch.zeros((3, 3), dtype=torch.uint8, device="cuda")),
                lambda: ops.voxel_downsample(two, 1.0, normals=torch.zeros((2, 3), device="cuda"))):
        with pytest.raises(UfrError):
            bad()
    p, c, n, count = ops.voxel_downsample(two, (1.0 + 1e-9) / (2 ** 21 - 5))     # the largest grid that is taken
    assert p.shape == (2, 3) and count.tolist() == [1, 1]


# ------------------------------------------------------------------ the whole filter and the command
def test_filter_points_counts_and_stages():
    rgb = np.random.default_rng(4).integers(0, 256, (len(CLOUD), 3)).astype(np.uint8)
    out = pcd_filter.filter_points(CLOUD, rgb, voxel_size=0.02, nb_neighbors=20, std_ratio=2.0, radius=0.5, nb_points=3, normals_k=16,
                                   viewpoints=VIEWS["two"])
    c = out["counts"]
    assert list(c) == ["input", "voxel", "statistical", "radius", "normals_valid"] and c["input"] == 2012
    assert c["statistical"] == c["voxel"] - 12 and c["radius"] == c["statistical"] == c["normals_valid"]
    assert len(out["points"]) == len(out["colors"]) == len(out["normals"]) == c["radius"]
    assert float(out["points"].norm(dim=1).max()) < 1.5
    out = pcd_filter.filter_points(CLOUD, nb_neighbors=0)
    assert out["counts"] == dict(input=2012) and out["normals"] is None and out["colors"] is None


def test_command_writes_clouds_that_the_other_commands_read(tmp_path, capsys):
    rng = np.random.default_rng(6)
    os.makedirs(tmp_path / "in" / "pcd")
    rgb = rng.integers(0, 256, (len(CLOUD), 3)).astype(np.uint8)
    depth_fusion.write_ply(str(tmp_path / "in" / "pcd" / "scan24.ply"), CLOUD.astype(np.float32), rgb)
    argv = ["--root_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--scans", "24", "37", "--voxel_size", "0.02",
            "--nb_neighbors", "20", "--std_ratio", "2", "--normals", "16"]
    assert pcd_filter.main(argv) == 0
    said = capsys.readouterr().out
    assert "scan37.ply" in said and "largest component" in said          # the missing scan, and the V = 0 rule, one line each
    report = json.load(open(tmp_path / "out" / "pcd_filter.json"))
    counts = report["scans"]["scan24"]
    assert list(report["scans"]) == ["scan24"] and counts["input"] == 2012 and counts["statistical"] == counts["voxel"] - 12
    path = str(tmp_path / "out" / "pcd" / "scan24.ply")
    header = open(path, "rb").read(400).split(b"end_header")[0].decode()
    assert "binary_little_endian" in header and "property float nx" in header and "property uchar red" in header
    v, f, c = dtu_eval.read_ply(path, with_colors=True)
    assert f is None and len(v) == counts["statistical"] == len(c)
    assert np.sqrt((v * v).sum(1)).max() < 1.5                           # the 12 far points are gone
    K = np.array([[40.0, 0, 16], [0, 40.0, 16], [0, 0, 1]])
    c2w = np.eye(4)
    c2w[2, 3] = -4.0
    img = RT.render_points(v, K, c2w, 32, 32, colors=c)
    assert img.shape == (1, 32, 32, 3) and img.dtype == np.uint8 and (img != 255).any()
    # named files go to <out_dir>/pcd/<stem>.ply
    assert pcd_filter.main(["--root_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out2"), "--ply", path, "--nb_neighbors", "0",
                            "--radius", "0.5", "--nb_points", "2"]) == 0
    v2, _, c2 = dtu_eval.read_ply(str(tmp_path / "out2" / "pcd" / "scan24.ply"), with_colors=True)
    assert len(v2) == len(v) and np.array_equal(c2, c)
