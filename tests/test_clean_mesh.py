"""DTU mesh cleaning (uforecon_amd/clean_mesh.py, csrc/mesh_clean.hip) against the reference's evaluation/clean_mesh.py.
tests/golden/clean_mesh_*.npz are recorded outputs of the reference's own functions (tests/golden/make_golden_clean_mesh.py
states the stubs); clean_mesh_ref.py restates the four stages in numpy.  CPU tests pin the restatement to the recorded run;
GPU tests pin the kernels to the restatement.

First-hit images are compared on every pixel that is not *close* by the restatement's own margins (clean_mesh_ref.py: a
barycentric coordinate within 1e-6 of an edge, or two hits within 1e-6 relative in t).  The ray generator and the edge
functions are the same expressions in the kernel and in the restatement, so elsewhere the face ids must be equal; the
``sphere3`` fixture has no close pixel at all (the generator asserts it), so there the whole pipeline must match exactly.

Union-find rounds: a 4 096-face strip is one chain.  Label propagation needs about one round per face.  Here a round hooks the
larger of two roots under the smaller and then jumps every face to its root: an index-ordered chain is linked in one round
and confirmed by an idle one, and in any order the roots that survive a round are local minima among their neighbouring
trees, about a third of them on a randomly ordered chain.  A hook lost to a lower concurrent one is repeated in the next
round.  The bound asserted is 2 log2(4096) = 24 rounds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clean_mesh_ref as R
from uforecon_amd import _lib, clean_mesh as CM, dtu_eval, ops
from uforecon_amd._lib import UfrError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = ("sphere3", "edges")
VIEWS = [23, 24, 33]


def load_golden(name):
    g = dict(np.load(os.path.join(HERE, "golden", f"clean_mesh_{name}.npz")))
    g["cams"] = [(g[f"K_{i}"], g[f"E_{i}"]) for i in range(3)]
    g["masks"] = [g[f"mask_{i}"] for i in range(3)]
    return g


_restated = {}


def restated(name):
    """the restatement's run of a golden fixture, computed once and shared (never modified)"""
    if name not in _restated:
        g = load_golden(name)
        _restated[name] = (g, R.clean_mesh(g["verts"], g["faces"], g["cams"], g["masks"], min_faces=int(g["min_faces"])))
    return _restated[name]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from uforecon_amd.build import build_library

        build_library(verbose=False)
    return _lib.load()


def latlong_sphere(nlat, nlon, radius=1.0, centre=(0.0, 0.0, 0.0)):
    v = [(0.0, 1.0, 0.0)]
    for i in range(1, nlat):
        for j in range(nlon):
            th, ph = np.pi * i / nlat, 2 * np.pi * j / nlon
            v.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon   # noqa: E731
    f = []
    for j in range(nlon):
        f.append((0, ring(1, j + 1), ring(1, j)))
        f.append((len(v) - 1, ring(nlat - 1, j), ring(nlat - 1, j + 1)))
    for i in range(1, nlat - 1):
        for j in range(nlon):
            f.append((ring(i, j), ring(i, j + 1), ring(i + 1, j)))
            f.append((ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)))
    return np.asarray(v, np.float64) * radius + np.asarray(centre, np.float64), np.asarray(f, np.int32)


# ------------------------------------------------------------------ CPU: restatement == the reference's recorded outputs
@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_votes_and_stage2_equal_the_reference_run(name):
    g, r = restated(name)
    for k in (0, 1, 2):
        assert np.array_equal(r["votes"] > k, g[f"ref_keep_{k}"]), k
    assert r["verts2"].dtype == np.float64 and np.array_equal(r["verts2"], g["ref_verts2"])
    assert r["faces2"].dtype == np.int32 and np.array_equal(r["faces2"], g["ref_faces2"])
    assert 0 < len(r["faces2"]) < len(g["faces"])


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_cameras_and_rays_equal_the_reference_run(name):
    g = load_golden(name)
    H, W = g["masks"][0].shape
    for i, (K, E) in enumerate(g["cams"]):
        Kn, c2w = R.camera(K, E)
        assert np.abs(Kn - g[f"ref_K_{i}"][:3, :3]).max() <= 1e-5
        assert c2w.dtype == np.float32 and np.abs(c2w.astype(np.float64) - g[f"ref_pose_{i}"]).max() <= 1e-5
        o, d = R.rays(R.k_inverse(Kn), c2w, H, W)
        assert np.abs(d.reshape(-1, 3).astype(np.float64) - g[f"ref_rays_v_{i}"]).max() <= 2e-6
        assert np.abs(o.astype(np.float64) - g[f"ref_rays_o_{i}"]).max() <= 2e-6
        # the product forms the same two matrices
        k_inv, c2w_p = CM.ray_camera(K, E)
        assert np.array_equal(k_inv, R.k_inverse(Kn)) and np.array_equal(c2w_p, c2w)
        assert np.array_equal(CM.projection(K, E), R.projection(K, E))


def test_sphere3_fixture_is_what_the_issue_describes():
    g, r = restated("sphere3")
    assert len(g["faces"]) == 2208 + 528 + 300 + 80 and all(m.shape == (48, 64) for m in g["masks"])
    assert sum(int(c.sum()) for c in r["close"]) == 0                      # no close pixel: the pipeline must match exactly
    assert len(r["faces2"]) == 2208 + 528 + 80                              # the blob lost the vote
    assert 0 < len(r["faces"]) < len(r["faces3"]) < len(r["faces2"])        # first hit and min_faces both remove faces
    assert (np.bincount(r["labels"][r["labels"] >= 0]) > 0).sum() > 1 and (r["labels"] == -1).any()


@pytest.mark.parametrize("k,want", [(1, [0]), (3, [0, 1, 0]), (11, [0, 3, 4, 5, 5, 5, 5, 5, 4, 3, 0])])
def test_element_table(lib, k, want):
    assert R.half_widths(k) == want
    assert ops.mask_half_widths(k) == want and CM.ellipse_half_widths(k) == want
    assert R.ellipse(k).sum() == sum(2 * w + 1 for w in want)


def test_dilation_restatement_on_a_hand_computed_image():
    img = np.zeros((7, 9), np.uint8)
    img[0, 0], img[3, 4] = 200, 90
    d = R.dilate(img, 3)                                                    # the 3 x 3 ellipse is a cross
    assert d[0, 1] == 200 and d[1, 0] == 200 and d[1, 1] == 0 and d[3, 5] == 90 and d[2, 4] == 90 and d[2, 3] == 0
    assert np.array_equal(R.dilate(img, 1), img)
    assert R.dilated_mask(img, 3).sum() == 3


def test_ply_round_trips_through_the_evaluation_reader(tmp_path):
    v, f = latlong_sphere(4, 5)
    CM.write_ply(str(tmp_path / "m.ply"), v, f)
    rv, rf = dtu_eval.read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(rv, v.astype(np.float32).astype(np.float64)) and np.array_equal(rf, f) and rf.dtype == np.int32
    head = open(tmp_path / "m.ply", "rb").read(200)
    assert b"binary_little_endian" in head and b"property float x" in head and b"property list uchar int vertex_indices" in head
    CM.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    rv, rf = dtu_eval.read_ply(str(tmp_path / "e.ply"))
    assert rv.shape == (0, 3) and len(rf) == 0


def test_lib_signatures_match_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ufr.h")).read(), flags=re.S)
    found = 0
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_(?:mask|mesh)_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        found += 1
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is (C.c_size_t if res == "size_t" else C.c_int), name
        want = [p.strip() for p in params.split(",")]
        assert len(want) == len(args), name
        for p, a in zip(want, args):
            if "*" in p or p.startswith("ufr_stream"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}[p.split()[0]], (name, p)
    assert found == 8 + 3                      # the eight of mesh cleaning and ufr_mesh_sample_* of the chamfer evaluation
    assert _lib.ABI_VERSION == 507 and "#define UFR_ABI_VERSION 507" in open(os.path.join(ROOT, "include", "ufr.h")).read()


def test_abi_rejects_bad_arguments(lib):
    hw = (C.c_int32 * 16)()
    assert lib.ufr_mask_half_widths(4, hw) == -1 and b"odd" in lib.ufr_last_error()
    assert lib.ufr_mask_half_widths(129, hw) == -1
    assert lib.ufr_mask_dilate(None, 4, 4, 3, 128, None, None, None) == -1 and b"null" in lib.ufr_last_error()
    assert lib.ufr_mesh_vertex_votes(None, 1, None, None, 3, 4, 4, None, None) == -1
    assert lib.ufr_mesh_first_hit_workspace_bytes(0, 4, 4) == 0 and lib.ufr_mesh_first_hit_workspace_bytes(10, 48, 64) >= 48 * 64 * 8 + 44
    assert lib.ufr_mesh_first_hit(None, None, 1, 1, None, None, None, 4, 4, None, None, None, 0, None) == -1
    assert lib.ufr_mesh_edge_keys(None, None, 1, 1, None, None) == -1
    assert lib.ufr_mesh_face_components_workspace_bytes(0) == 0 and lib.ufr_mesh_face_components_workspace_bytes(2 ** 30) == 0
    assert lib.ufr_mesh_face_components(None, None, 1, None, None, 0, None, None) == -1


def test_command_line_takes_the_reference_flags():
    a = CM.make_parser().parse_args([])
    assert (a.root_dir, a.out_dir, a.n_view, a.set, a.scale_factor) == ("./dtu_test", "./outputs/mesh", 3, 0, None)
    assert a.test_ref_view == [23, 24, 33, 22, 15, 34, 14, 32, 16, 35, 25] and a.min_faces == 500
    assert a.scans == [24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122]
    a = CM.make_parser().parse_args("--set 1 --n_view 4 --scale_factor 2.5 --scans 24 37 --min_faces 7".split())
    assert (a.set, a.n_view, a.scale_factor, a.scans, a.min_faces) == (1, 4, 2.5, [24, 37], 7)


def test_scale_factor_cancels_in_the_ray_camera(tmp_path):
    g = load_golden("sphere3")
    K, E = g["cams"][1]
    with open(tmp_path / "c.txt", "w") as f:
        f.write("extrinsic\n" + "\n".join(" ".join("%.9g" % x for x in row) for row in E) + "\n\nintrinsic\n"
                + "\n".join(" ".join("%.9g" % x for x in row) for row in K) + "\n\n0 1\n")
    K1, E1 = CM.read_cam_file(str(tmp_path / "c.txt"))
    assert np.array_equal(K1, K) and np.array_equal(E1, E)
    K2, E2 = CM.read_cam_file(str(tmp_path / "c.txt"), scale_factor=4.0)          # a power of two: exact
    assert np.array_equal(E2, E / 4)
    for a, b in zip(CM.ray_camera(K1, E1), CM.ray_camera(K2, E2)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        CM.read_cam_file(str(tmp_path / "c.txt"), scale_factor=-1.0)


# ------------------------------------------------------------------ GPU
def cuda(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


EXACT_K = np.array([[16, 0, 32], [0, 16, 24], [0, 0, 1]], np.float32)          # powers of two: an exact inverse
EXACT_E = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 3], [0, 0, 0, 1]], np.float32)   # at (0, 0, 3), looking down -z


def gpu_first_hit(verts, faces, K, E, mask):
    k_inv, c2w = CM.ray_camera(K, E)
    fid, hit = ops.mesh_first_hit(cuda(np.asarray(verts, np.float64)), cuda(np.asarray(faces, np.int32).reshape(-1, 3)), k_inv, c2w,
                                  cuda(np.asarray(mask, np.uint8)))
    fid, hit = fid.cpu().numpy(), hit.cpu().numpy()
    want = np.zeros(len(hit), np.uint8)
    want[fid[fid >= 0]] = 1
    assert np.array_equal(hit, want)
    return fid


def ref_first_hit(verts, faces, K, E, mask):
    Kn, c2w = R.camera(K, E)
    return R.first_hit(verts, faces, R.k_inverse(Kn), c2w, mask, return_close=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 11])
def test_dilation_is_exact_borders_included(k):
    rng = np.random.default_rng(k)
    img = rng.integers(0, 256, (37, 53)).astype(np.uint8)
    img[rng.random((37, 53)) < 0.8] = 0                                     # sparse: the element's shape shows
    img[0, 0], img[36, 52], img[0, 52], img[36, 0] = 255, 250, 129, 128
    mask, dil = ops.dilate_mask(cuda(img), k, return_dilated=True)
    want = R.dilate(img, k)
    assert np.array_equal(dil.cpu().numpy(), want)
    assert np.array_equal(mask.cpu().numpy(), (want > 128).astype(np.uint8))
    assert np.array_equal(ops.dilate_mask(cuda(img), k, threshold=10).cpu().numpy(), (want > 10).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_votes_are_exact_against_the_goldens(name):
    g, r = restated(name)
    dil = np.stack([R.dilated_mask(m) for m in g["masks"]]).astype(np.uint8)
    P = np.stack([R.projection(K, E) for K, E in g["cams"]])
    for Pin in (P, P[:, :3]):
        votes = ops.mesh_vertex_votes(cuda(g["verts"]), cuda(Pin), cuda(dil)).cpu().numpy()
        assert votes.dtype == np.int32 and np.array_equal(votes, r["votes"])
    for k in (0, 1, 2):
        assert np.array_equal(votes > k, g[f"ref_keep_{k}"])


@pytest.mark.gpu
def test_first_hit_equals_the_restatement_on_sphere3():
    g, r = restated("sphere3")
    n = 0
    for (K, E), m, want, close in zip(g["cams"], r["dilated"], r["face_ids"], r["close"]):
        fid = gpu_first_hit(r["verts2"], r["faces2"], K, E, m)
        assert np.array_equal(fid[~close], want[~close])
        assert (fid[~m] == -1).all()
        n += int((fid >= 0).sum())
    assert n > 3000


@pytest.mark.gpu
def test_first_hit_planar_grid_on_pixel_centres_has_no_cracks():
    """8 x 8 x 2 triangles whose vertices project exactly onto pixel centres (every 4th pixel): rays run exactly through
    vertices, along the axis-parallel and along the diagonal edges"""
    px, py = np.meshgrid(16 + 4 * np.arange(9), 8 + 4 * np.arange(9))
    verts = np.stack([(px.ravel() - 32) / 8.0, -(py.ravel() - 24) / 8.0, np.ones(81)], 1)     # depth 2: pixel = 8 x + 32
    faces = []
    for j in range(8):
        for i in range(8):
            a = 9 * j + i
            faces += [(a, a + 1, a + 9), (a + 10, a + 9, a + 1)]
    faces = np.asarray(faces, np.int32)
    mask = np.ones((48, 64), np.uint8)
    mask[::5, ::7] = 0
    fid = gpu_first_hit(verts, faces, EXACT_K, EXACT_E, mask)
    Kn, c2w = R.camera(EXACT_K, EXACT_E)
    o, d = R.rays(R.k_inverse(Kn), c2w, 48, 64)
    t32, near = R.hit_table(verts, faces, o, d.reshape(-1, 3))
    contains = np.isfinite(t32).reshape(48, 64, -1)
    ys, xs = np.mgrid[:48, :64]
    inner = (xs > 16) & (xs < 48) & (ys > 8) & (ys < 40)
    outer = (xs < 16) | (xs > 48) | (ys < 8) | (ys > 40)                   # the pixels on the rim itself may go either way
    assert contains.any(-1)[inner].all() and not contains.any(-1)[outer].any()      # the restatement itself has no crack
    rays = inner & (mask != 0)
    assert (fid[rays] >= 0).all() and (fid[outer | (mask == 0)] == -1).all()
    assert contains[ys[rays], xs[rays], fid[rays]].all()
    assert near.reshape(48, 64, -1).any(-1)[rays].sum() >= 7 * 7 - 10       # the rays through the inner vertices are near-edge
    want = R.first_hit(verts, faces, R.k_inverse(Kn), c2w, mask)
    assert np.array_equal(fid, want)                                        # same expressions: equal even on the edges


@pytest.mark.gpu
def test_first_hit_large_straddling_degenerate_and_coincident_triangles():
    mask = np.ones((48, 64), np.uint8)
    # one triangle covering the whole image: the cooperative path
    big = np.array([[-40.0, -30.0, 0.0], [40.0, -30.0, 0.0], [0.0, 50.0, 0.0]])
    fid = gpu_first_hit(big, [[0, 1, 2]], EXACT_K, EXACT_E, mask)
    assert (fid == 0).all()
    g = load_golden("sphere3")
    for K, E in g["cams"]:
        want, close = ref_first_hit(big, [[0, 1, 2]], K, E, mask)
        fid = gpu_first_hit(big, [[0, 1, 2]], K, E, mask)
        assert np.array_equal(fid[~close], want[~close]) and (want == 0).all()
    # one triangle straddling the camera plane (the third vertex is behind camera 0 at z = 3): no projected box
    strad = np.array([[-1.5, -1.0, 0.0], [1.2, -1.1, 0.0], [0.1, 0.4, 6.0]])
    want, close = ref_first_hit(strad, [[0, 1, 2]], EXACT_K, EXACT_E, mask)
    fid = gpu_first_hit(strad, [[0, 1, 2]], EXACT_K, EXACT_E, mask)
    assert np.array_equal(fid[~close], want[~close]) and close.mean() < 0.01
    assert 100 < (want == 0).sum() < 48 * 64 - 100
    # ... and one wholly behind it is never hit
    assert (gpu_first_hit(strad + [0, 0, 7.0], [[0, 1, 2]], EXACT_K, EXACT_E, mask) == -1).all()
    # zero-area triangles (a repeated vertex; three collinear points) in front of a real one are never hit
    v = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0], [-1.0, -1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0]])
    f = [[3, 4, 4], [3, 5, 4], [0, 1, 2]]
    fid = gpu_first_hit(v, f, EXACT_K, EXACT_E, mask)
    assert set(np.unique(fid)) == {-1, 2} and np.array_equal(fid, R.first_hit(v, f, *_kc(EXACT_K, EXACT_E), mask))
    # of two coincident triangles the lower index wins, whatever the pixel
    f = [[0, 1, 2], [0, 1, 2], [3, 4, 4]]
    fid = gpu_first_hit(v, f, EXACT_K, EXACT_E, mask)
    assert set(np.unique(fid)) == {-1, 0} and np.array_equal(fid, R.first_hit(v, f, *_kc(EXACT_K, EXACT_E), mask))
    assert (fid == 0).sum() == 61                                           # the triangle's pixels (counted by the restatement)
    f = [[3, 4, 4], [0, 1, 2], [0, 1, 2]]
    assert set(np.unique(gpu_first_hit(v, f, EXACT_K, EXACT_E, mask))) == {-1, 1}


def _kc(K, E):
    Kn, c2w = R.camera(K, E)
    return R.k_inverse(Kn), c2w


def gpu_components(verts, faces, **kw):
    out = ops.mesh_face_components(cuda(np.asarray(verts, np.float64)), cuda(np.asarray(faces, np.int32).reshape(-1, 3)), **kw)
    return (out[0].cpu().numpy(), out[1]) if kw else out.cpu().numpy()


@pytest.mark.gpu
def test_components_spheres_fans_and_soups():
    v1, f1 = latlong_sphere(24, 48)
    v2, f2 = latlong_sphere(7, 9, 0.3, (3.0, 0.0, 0.0))
    verts, faces = np.concatenate([v1, v2]), np.concatenate([f1, f2 + len(v1)])
    labels = gpu_components(verts, faces)
    assert labels.dtype == np.int32 and (labels[:len(f1)] == 0).all() and (labels[len(f1):] == len(f1)).all()
    assert np.array_equal(labels, R.components(verts, faces))
    # an edge that three faces share gives no adjacency; a lone pair beside them does
    fan_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [5, 0, 0], [6, 0, 0], [5, 1, 0], [6, 1, 0]], np.float64)
    fan_f = [[0, 1, 2], [0, 1, 3], [1, 0, 4], [5, 6, 7], [6, 8, 7], [2, 2, 4]]
    assert gpu_components(fan_v, fan_f).tolist() == [-1, -1, -1, 3, 3, -1] == R.components(fan_v, fan_f).tolist()
    # a duplicated-vertex soup of the sphere (every face its own three vertices), faces shuffled: the same components after merging
    perm = np.random.default_rng(0).permutation(len(faces))
    soup_v = verts[faces[perm]].reshape(-1, 3)
    soup_f = np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)
    ls = gpu_components(soup_v, soup_f)
    assert np.array_equal(ls, R.components(soup_v, soup_f))
    big = perm < len(f1)
    assert len(np.unique(ls)) == 2 and len(np.unique(ls[big])) == 1 and ls[big][0] == np.flatnonzero(big)[0]
    # the same bits run after run
    for _ in range(2):
        assert np.array_equal(gpu_components(soup_v, soup_f), ls)


@pytest.mark.gpu
def test_components_of_a_4096_face_strip_converge_in_a_few_rounds():
    n = 4096
    x = np.arange(n // 2 + 1, dtype=np.float64)
    verts = np.concatenate([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 1, 0 * x], 1)])
    top = n // 2 + 1
    faces = np.empty((n, 3), np.int32)
    i = np.arange(n // 2)
    faces[0::2] = np.stack([i, i + 1, top + i], 1)
    faces[1::2] = np.stack([i + 1, top + i + 1, top + i], 1)
    labels, rounds = gpu_components(verts, faces, return_rounds=True)
    assert (labels == 0).all()
    print("rounds", rounds)
    assert 2 <= rounds <= 24
    # the chain in a shuffled face order: still one component, labelled by its lowest face
    perm = np.random.default_rng(1).permutation(n)
    labels, rounds2 = gpu_components(verts, faces[perm], return_rounds=True)
    print("rounds (shuffled)", rounds2)
    assert (labels == 0).all() and rounds2 <= 24


@pytest.mark.gpu
def test_clean_mesh_equals_the_restatement_on_sphere3_and_is_repeatable():
    g, r = restated("sphere3")
    kw = dict(min_faces=int(g["min_faces"]))
    v, f, st = CM.clean_mesh(g["verts"], g["faces"], g["cams"], g["masks"], return_stages=True, **kw)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v, r["verts"]) and np.array_equal(f, r["faces"])
    assert np.array_equal(st["votes"], r["votes"])
    assert np.array_equal(st["verts2"], r["verts2"]) and np.array_equal(st["faces2"], r["faces2"])
    assert np.array_equal(st["verts2"], g["ref_verts2"]) and np.array_equal(st["faces2"], g["ref_faces2"])
    for a, b in zip(st["face_ids"], r["face_ids"]):
        assert np.array_equal(a, b)
    assert np.array_equal(st["faces3"], r["faces3"]) and np.array_equal(st["labels"], r["labels"])
    # return_stages is consistent with itself and with the plain call
    hit = np.zeros(len(st["faces2"]), bool)
    for a in st["face_ids"]:
        hit[a[a >= 0]] = True
    assert np.array_equal(st["faces2"][hit], st["faces3"]) and st["rounds"] >= 1
    v2, f2 = CM.clean_mesh(g["verts"].astype(np.float64), g["faces"].astype(np.int64), g["cams"], g["masks"], **kw)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    # the largest component only
    vl, fl = CM.clean_mesh(g["verts"], g["faces"], g["cams"], g["masks"], min_faces=1, largest_only=True)
    wl = R.clean_mesh(g["verts"], g["faces"], g["cams"], g["masks"], min_faces=1, largest_only=True)
    assert np.array_equal(vl, wl["verts"]) and np.array_equal(fl, wl["faces"])


@pytest.mark.gpu
def test_command_line_on_a_dtu_shaped_tree(tmp_path, capsys):
    from PIL import Image

    g, r = restated("sphere3")
    root, out = tmp_path / "dtu", tmp_path / "out" / "mesh"
    os.makedirs(root / "cameras")
    os.makedirs(root / "scan24" / "mask")
    os.makedirs(out)
    for vid, (K, E), m in zip(VIEWS, g["cams"], g["masks"]):
        with open(root / "cameras" / "{:0>8}_cam.txt".format(vid), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join("%.9g" % x for x in row) for row in E) + "\n\nintrinsic\n"
                    + "\n".join(" ".join("%.9g" % x for x in row) for row in K) + "\n\n0 1\n")
        Image.fromarray(np.stack([np.zeros_like(m), 255 - m, m], -1)).save(root / "scan24" / "mask" / "{:0>3}.png".format(vid))
        assert np.array_equal(CM.read_mask(str(root / "scan24" / "mask" / "{:0>3}.png".format(vid))), m)   # the blue channel
    CM.write_ply(str(out / "scan24.ply"), g["verts"], g["faces"])
    CM.main(["--root_dir", str(root), "--out_dir", str(out), "--scans", "24", "37", "--min_faces", "100"])
    text = capsys.readouterr().out
    assert "processing scan24" in text and "finish processing scan24" in text and "scan37 is empty" in text
    for name in ("clean_024.ply", "scan24_raw.ply", "scan24.ply"):
        assert (out / "final" / name).exists(), name
    assert not (out / "final" / "scan37.ply").exists()
    v, f = dtu_eval.read_ply(str(out / "final" / "scan24.ply"))
    # the file holds float32 vertices: the same call on them
    v32 = g["verts"].astype(np.float32).astype(np.float64)
    wv, wf = CM.clean_mesh(v32, g["faces"], g["cams"], g["masks"], min_faces=100)
    assert len(f) > 0 and np.array_equal(f, wf) and np.array_equal(v, wv.astype(np.float32).astype(np.float64))
    v2, f2 = dtu_eval.read_ply(str(out / "final" / "clean_024.ply"))
    vr, fr = dtu_eval.read_ply(str(out / "final" / "scan24_raw.ply"))
    assert len(v2) == len(vr) and len(f) < len(fr) < len(f2)


@pytest.mark.gpu
def test_errors_and_empty_results():
    import torch

    g = load_golden("sphere3")
    verts, faces, cams, masks = g["verts"], g["faces"], g["cams"], g["masks"]
    bad = faces.copy()
    bad[5, 1] = len(verts)
    with pytest.raises(UfrError, match="face indices"):
        CM.clean_mesh(verts, bad, cams, masks)
    k_inv, c2w = CM.ray_camera(*cams[0])
    with pytest.raises(UfrError, match="face indices"):
        ops.mesh_first_hit(cuda(verts), cuda(bad), k_inv, c2w, cuda(masks[0]))
    bad[5, 1] = -1
    with pytest.raises(UfrError, match="face indices"):
        ops.mesh_face_components(cuda(verts), cuda(bad))
    with pytest.raises(UfrError, match="one size"):
        CM.clean_mesh(verts, faces, cams, [masks[0], masks[1], masks[2][:40]])
    with pytest.raises(UfrError, match="one mask per camera"):
        CM.clean_mesh(verts, faces, cams, masks[:2])
    with pytest.raises(UfrError):
        ops.mesh_vertex_votes(cuda(verts), cuda(np.zeros((3, 3, 4), np.float32)), cuda(np.zeros((2, 48, 64), np.uint8)))
    with pytest.raises(UfrError):
        ops.dilate_mask(cuda(masks[0]), 4)
    with pytest.raises(UfrError):
        ops.dilate_mask(torch.from_numpy(masks[0]), 11)                     # a host tensor
    with pytest.raises(UfrError):
        ops.mesh_first_hit(cuda(verts.astype(np.float32)), cuda(faces), k_inv, c2w, cuda(masks[0]))
    # an empty mesh, masks without a ray, nothing surviving: empty arrays
    for v, f, m, kw in ((np.zeros((0, 3)), np.zeros((0, 3), np.int32), masks, {}),
                        (verts, np.zeros((0, 3), np.int32), masks, {}),
                        (verts, faces, [np.zeros_like(x) for x in masks], {}),
                        (verts, faces, masks, dict(min_faces=10 ** 6))):
        ov, of, st = CM.clean_mesh(v, f, cams, m, return_stages=True, **kw)
        assert ov.shape == (0, 3) and ov.dtype == np.float64 and of.shape == (0, 3) and of.dtype == np.int32
        assert len(st["face_ids"]) == 3 and all(a.shape == (48, 64) for a in st["face_ids"])
    # masks without a ray: the ones border still votes for nothing inside the image
    fid, hit = ops.mesh_first_hit(cuda(verts), cuda(faces), k_inv, c2w, cuda(np.zeros((48, 64), np.uint8)))
    assert int((fid != -1).sum()) == 0 and int(hit.sum()) == 0
