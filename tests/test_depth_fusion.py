"""Depth-map fusion to a point cloud (uforecon_amd/depth_fusion.py, csrc/depth_fusion.hip) against the reference's
code1/encoder_utils/depth_fusion.py.  tests/golden/depth_fusion_*.npz are recorded runs of the reference module
(tests/golden/make_golden_depth_fusion.py; its cv2.remap is the numpy statement of tests/depth_fusion_ref.py, no OpenCV being
at hand); depth_fusion_ref.py restates the interface in numpy.  CPU tests pin the restatement to the recorded run bit for
bit; GPU tests pin the kernels to both.

The near-threshold exemption is a condition on the reference's own margins, not a measurement of the kernels: a (pair, pixel)
is *close* when |dist - geo_pixel_thres| < 1e-3 or |relative_depth_diff - geo_depth_thres| < 1e-5 (about ten fp32 ulps of a
coordinate below 2048, 1.2e-4 px, and of a relative depth, 6e-8).  Per-pair masks must equal the reference on every other
pair; a pixel none of whose pairs is close must match in geo_mask_sum, geo_mask, depth_est_averaged (1 fp64 ulp: the sum is
fp32 in a fixed order), xyz (1 fp32 ulp) and rgb.  The fixtures' close share must stay below 0.5 %."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_fusion_ref as R
from uforecon_amd import _lib, depth_fusion as DF, dtu_eval, ops
from uforecon_amd._lib import UfrError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = ("full", "nview")
CLOSE_SHARE = 0.005


def load_golden(name):
    g = dict(np.load(os.path.join(HERE, "golden", f"depth_fusion_{name}.npz")))
    n = int(g["n_views"])
    g["depths"] = [g[f"depth_{v}"] for v in range(n)]
    g["Ks"] = [g[f"K_{v}"] for v in range(n)]
    g["Es"] = [g[f"E_{v}"] for v in range(n)]
    g["colors"] = [g[f"color_{v}"] for v in range(n)]
    off = np.concatenate([[0], np.cumsum(g["pair_len"])])
    g["pairs"] = [(int(r), [int(s) for s in g["pair_src"][off[i]:off[i + 1]]]) for i, r in enumerate(g["pair_ref"])]
    pt = float(g["geo_pixel_thres"])
    g["kw"] = dict(geo_pixel_thres=int(pt) if pt == int(pt) else pt, geo_depth_thres=float(g["geo_depth_thres"]),
                   geo_mask_thres=int(g["geo_mask_thres"]))
    g["masks"] = [np.unpackbits(g[f"mask_{i}"])[:g["depths"][r].size].reshape(g["depths"][r].shape).astype(bool)
                  for i, (r, _) in enumerate(g["pairs"])]
    return g


_restated = {}


def restated(name):
    """the restatement's run of a golden fixture, computed once and shared (never modified)"""
    if name not in _restated:
        g = load_golden(name)
        _restated[name] = (g, R.fuse_views(g["depths"], g["Ks"], g["Es"], g["colors"], g["pairs"], **g["kw"]))
    return _restated[name]


def within_ulp(a, b, n=1):
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.abs(a - b) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from uforecon_amd.build import build_library

        build_library(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------ CPU: restatement == the reference's recorded run
@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_matches_the_reference_run_bit_for_bit(name):
    g, (xyz, rgb, masks, details) = restated(name)
    assert len(masks) == len(g["pairs"])
    for i, (mask, d) in enumerate(zip(masks, details)):
        assert np.array_equal(mask, g["masks"][i]), i
        assert d["geo_mask_sum"].dtype == np.int32 and np.array_equal(d["geo_mask_sum"], g[f"geo_mask_sum_{i}"]), i
        assert d["depth_est_averaged"].dtype == np.float64
        assert np.array_equal(d["depth_est_averaged"][mask], g[f"depth_avg_valid_{i}"]), i
        # the margins (float32 in the fixture; NaN and inf where the reference has them)
        assert np.array_equal(d["dist"].astype(np.float32), g[f"dist_{i}"], equal_nan=True), i
        assert np.array_equal(d["relative_depth_diff"], g[f"rel_{i}"], equal_nan=True), i
    assert xyz.dtype == np.float32 and np.array_equal(xyz, g["verts"])
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, g["vert_colors"])


def test_golden_exercises_every_branch():
    """what the fixture's maker asserted on the reference's record, recomputed from the fixture"""
    g = load_golden("full")
    pt, dt = g["kw"]["geo_pixel_thres"], np.float32(g["kw"]["geo_depth_thres"])
    n = pix = dep = close = 0
    for i, (ref, srcs) in enumerate(g["pairs"]):
        nz = (g["depths"][ref] != 0)[None]
        dist, rel = g[f"dist_{i}"], g[f"rel_{i}"]
        with np.errstate(invalid="ignore"):
            n += int(nz.sum()) * len(srcs)
            pix += int((nz & ~(dist < pt) & (rel < dt)).sum())
            dep += int((nz & (dist < pt) & ~(rel < dt)).sum())
            close += int((nz & R.close_pairs(dist, rel, pt, float(dt))).sum())
    assert pix / n >= 0.02 and dep / n >= 0.02 and close / n <= CLOSE_SHARE
    kept = sum(int(m.sum()) for m in g["masks"]) / sum(m.size for m in g["masks"])
    assert 0.10 <= kept <= 0.90
    assert any(not m.any() for m in g["masks"])                                        # a view with no valid pixel
    assert any(g["depths"][r].shape != g["depths"][s].shape for r, ss in g["pairs"] for s in ss)
    assert sorted(len(s) for _, s in g["pairs"])[0] == 1 and max(len(s) for _, s in g["pairs"]) == 10


def test_remap_restatement_on_hand_computed_taps():
    src = np.array([[1, 2, 4], [8, 16, 32]], np.float32)
    x = np.array([0.0, 0.5, 1.25, -0.5, 2.5, 2.0, -1.0, np.nan, np.inf, 1e12, 0.015], np.float32)
    y = np.array([0.0, 0.0, 0.50, 0.0, 1.0, 1.5, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32)
    want = [1, 1.5, 0.5 * (0.75 * 2 + 0.25 * 4) + 0.5 * (0.75 * 16 + 0.25 * 32), 0.5, 16, 16, 0, 0, 0, 0, 1]
    assert np.array_equal(R.remap(src, x, y), np.array(want, np.float32))      # 0.015 * 32 = 0.48 rounds to 0: 1/32 pixel steps
    assert np.array_equal(R.taps_outside(src.shape, x, y), [0, 0, 0, 2, 3, 3, 2, 4, 4, 4, 0])


def test_ply_round_trips_through_the_evaluation_reader(tmp_path):
    g = load_golden("full")
    p = str(tmp_path / "cloud.ply")
    DF.write_ply(p, g["verts"], g["vert_colors"])
    raw = open(p, "rb").read()
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(g["verts"]))
    assert raw.startswith(head) and len(raw) == len(head) + 15 * len(g["verts"])
    v, f = dtu_eval.read_ply(p)
    assert f is None and np.array_equal(v, g["verts"].astype(np.float64))
    rec = np.frombuffer(raw[len(head):], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert np.array_equal(rec["rgb"], g["vert_colors"])
    DF.write_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    v, f = dtu_eval.read_ply(p)
    assert f is None and v.shape == (0, 3)


def test_read_pair_file(tmp_path):
    p = tmp_path / "pair.txt"
    p.write_text("4\n0\n3 1 92.5 2 80.1 3 7.0\n1\n0\n2\n1 0 55.0 \n3\n10 0 9 1 8 2 7 0 6 1 5 2 4 0 3 1 2 2 1 3 0\n")
    assert DF.read_pair_file(str(p)) == [(0, [1, 2, 3]), (2, [0]), (3, [0, 1, 2, 0, 1, 2, 0, 1, 2, 3])]


def test_pair_matrices_keep_the_input_dtype_until_widened():
    g = load_golden("nview")
    K32, E32 = [k.astype(np.float32) for k in g["Ks"]], [e.astype(np.float32) for e in g["Es"]]
    m = DF.pair_matrices(K32[0], E32[0], K32[1], E32[1])
    assert m.dtype == np.float64 and m.shape == (ops.DEPTH_PAIR_DOUBLES,)
    assert np.array_equal(m[:9], np.linalg.inv(K32[0]).astype(np.float64).ravel())           # a float32 inverse, widened after
    assert np.array_equal(m[9:25], np.matmul(E32[1], np.linalg.inv(E32[0])).astype(np.float64).ravel())
    assert np.array_equal(m[25:34], K32[1].astype(np.float64).ravel()) and np.array_equal(m[59:], K32[0].astype(np.float64).ravel())
    m64 = DF.pair_matrices(g["Ks"][0], g["Es"][0], g["Ks"][1], g["Es"][1])
    assert np.array_equal(m64[43:59], np.matmul(g["Es"][0], np.linalg.inv(g["Es"][1])).ravel())
    assert np.array_equal(m64[34:43], np.linalg.inv(g["Ks"][1]).ravel())
    with pytest.raises(ValueError, match="3x3"):
        DF.pair_matrices(np.eye(4), np.eye(4), np.eye(3), np.eye(4))


def test_command_line_takes_the_reference_flags():
    a = DF.make_parser().parse_args([])
    assert (a.dataset, a.dataset_dir, a.root_dir, a.n_view, a.geo_pixel_thres, a.geo_depth_thres, a.geo_mask_thres, a.set,
            a.full_fusion) == ("DTU", None, None, 3, 1, 0.01, 2, 0, False)
    a = DF.make_parser().parse_args("--dataset X --dataset_dir d --root_dir r --n_view 5 --geo_pixel_thres 0.5 --geo_depth_thres 0.02 "
                                    "--geo_mask_thres 3 --set 1 --full_fusion".split())
    assert (a.dataset, a.dataset_dir, a.root_dir, a.n_view, a.geo_pixel_thres, a.geo_depth_thres, a.geo_mask_thres, a.set,
            a.full_fusion) == ("X", "d", "r", 5, 0.5, 0.02, 3, 1, True)
    with pytest.raises(ValueError, match="dataset_dir"):
        DF.filter_depth("nowhere", "scan1", full_fusion=True)


# ------------------------------------------------------------------ CPU: the C ABI's argument checks
def test_abi_rejects_bad_arguments(lib):
    fake = C.c_void_p(256)            # never dereferenced: validation returns before any device work
    err = lib.ufr_last_error
    ptrs = (C.c_void_p * 2)(256, 256)
    hw = (C.c_int32 * 4)(4, 5, 6, 7)

    def consistency(ref=fake, H=4, W=5, src=ptrs, shw=hw, mats=fake, S=2, msum=fake, mask=fake, avg=fake):
        return lib.ufr_depth_consistency(ref, H, W, src, shw, mats, S, 1.0, 0.01, 2, msum, mask, avg, None, None)

    for kw in (dict(ref=None), dict(src=None), dict(shw=None), dict(mats=None), dict(msum=None), dict(mask=None), dict(avg=None)):
        assert consistency(**kw) == -1
        assert b"ufr_depth_consistency" in err() and b"null" in err()
    assert consistency(src=(C.c_void_p * 2)(256, None)) == -1 and b"source 1" in err()
    assert consistency(H=0) == -1 and b"0x5" in err()
    assert consistency(W=-2) == -1 and b"4x-2" in err()
    assert consistency(H=65536, W=32768) == -1 and b"2^31" in err()
    assert consistency(S=0) == -1 and b"S 0" in err()
    assert consistency(S=ops.DEPTH_MAX_SOURCES + 1) == -1 and b"S 65" in err()
    assert consistency(shw=(C.c_int32 * 4)(4, 5, 0, 7)) == -1 and b"source 1 is 0x7" in err()
    assert lib.ufr_depth_consistency(fake, 4, 5, ptrs, hw, fake, 2, float("nan"), 0.01, 2, fake, fake, fake, None, None) == -1
    assert b"NaN" in err()

    assert lib.ufr_depth_points_workspace_bytes(0, 5) == 0 and lib.ufr_depth_points_workspace_bytes(5, 0) == 0
    assert lib.ufr_depth_points_workspace_bytes(65536, 32768) == 0
    need = lib.ufr_depth_points_workspace_bytes(70, 90)
    assert need >= 2 * 8 * ((70 * 90 + 255) // 256) + 8
    n = C.c_int64(0)
    assert lib.ufr_depth_points_count(None, 70, 90, fake, need, C.byref(n), None) == -1
    assert b"ufr_depth_points_count" in err() and b"null" in err()
    assert lib.ufr_depth_points_count(fake, 70, 90, None, need, C.byref(n), None) == -1 and b"null" in err()
    assert lib.ufr_depth_points_count(fake, 70, 90, fake, need, None, None) == -1 and b"n_host" in err()
    assert lib.ufr_depth_points_count(fake, 0, 90, fake, need, C.byref(n), None) == -1 and b"0x90" in err()
    assert lib.ufr_depth_points_count(fake, 65536, 32768, fake, need, C.byref(n), None) == -1 and b"2^31" in err()
    assert lib.ufr_depth_points_count(fake, 70, 90, fake, need - 1, C.byref(n), None) == -3 and b"workspace" in err()
    ik, ie = (C.c_double * 9)(), (C.c_double * 16)()

    def emit(mask=fake, avg=fake, col=fake, H=70, W=90, k=ik, e=ie, ws=fake, nb=need, xyz=fake, rgb=fake, cap=5):
        return lib.ufr_depth_points_emit(mask, avg, col, H, W, k, e, ws, nb, xyz, rgb, cap, None)

    for kw in (dict(mask=None), dict(avg=None), dict(col=None), dict(k=None), dict(e=None), dict(ws=None), dict(xyz=None), dict(rgb=None)):
        assert emit(**kw) == -1
        assert b"ufr_depth_points_emit" in err() and b"null" in err()
    assert emit(W=0) == -1 and b"70x0" in err()
    assert emit(cap=-1) == -1 and b"capacity" in err()
    assert emit(nb=need - 1) == -3 and b"workspace" in err()


def test_ops_refuse_host_tensors_and_wrong_dtypes(lib):
    import torch

    d = torch.zeros((4, 5), dtype=torch.float32)
    mats = torch.zeros((1, ops.DEPTH_PAIR_DOUBLES), dtype=torch.float64)
    with pytest.raises(UfrError, match="GPU"):
        ops.depth_consistency(d, [d], mats)
    with pytest.raises(UfrError, match="GPU"):
        ops.depth_points(torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((4, 5), dtype=torch.float64),
                         torch.zeros((4, 5, 3), dtype=torch.uint8), np.eye(3), np.eye(4))
    with pytest.raises(UfrError, match="tensor"):
        ops.depth_consistency(np.zeros((4, 5), np.float32), [d], mats)


# ------------------------------------------------------------------ GPU helpers
def gpu_fuse(depths, Ks, Es, colors, pairs, **kw):
    return DF.fuse_views(depths, Ks, Es, colors, pairs, return_details=True, **kw)


def assert_fusion_matches(got, want, depths, pairs, kw, max_close=None):
    """``got`` (the device) against ``want`` (the reference's record or the restatement, with its margins) under the
    module docstring's contract.  Returns the share of close (pair, pixel)s."""
    xyz_g, rgb_g, masks_g, det_g = got
    xyz_w, rgb_w, masks_w, det_w = want
    assert xyz_g.dtype == np.float32 and rgb_g.dtype == np.uint8
    assert len(xyz_g) == len(rgb_g) == sum(int(m.sum()) for m in masks_g)               # N = the masks' popcount
    n_pairs = n_close = 0
    og = ow = 0
    for i, (ref, srcs) in enumerate(pairs):
        dg, dw = det_g[i], det_w[i]
        close = R.close_pairs(dw["dist"], dw["relative_depth_diff"], kw["geo_pixel_thres"], kw["geo_depth_thres"])
        n_pairs += close.size
        n_close += int(close.sum())
        assert dg["pair_masks"].shape == dw["pair_masks"].shape
        assert np.array_equal(dg["pair_masks"][~close], dw["pair_masks"][~close]), f"view {ref}: a per-pair mask differs"
        calm = ~close.any(0)                                                             # pixels none of whose pairs is close
        assert np.array_equal(dg["geo_mask_sum"][calm], dw["geo_mask_sum"][calm]), f"view {ref}: geo_mask_sum"
        assert np.array_equal(masks_g[i][calm], masks_w[i][calm]), f"view {ref}: geo_mask"
        assert np.array_equal(masks_g[i], dg["geo_mask_sum"] >= kw["geo_mask_thres"])
        a, b = dg["depth_est_averaged"][calm], dw["depth_est_averaged"][calm]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin) and within_ulp(a[fin], b[fin]).all(), f"view {ref}: depth_est_averaged"
        # the clouds: row-major selection, compared index by index on the calm pixels both hold
        ng, nw = int(masks_g[i].sum()), int(masks_w[i].sum())
        both = masks_g[i] & masks_w[i] & calm
        ig = (np.cumsum(masks_g[i].ravel()) - 1).reshape(masks_g[i].shape)[both] + og
        iw = (np.cumsum(masks_w[i].ravel()) - 1).reshape(masks_w[i].shape)[both] + ow
        assert within_ulp(xyz_g[ig], xyz_w[iw]).all(), f"view {ref}: xyz"
        assert np.array_equal(rgb_g[ig], rgb_w[iw]), f"view {ref}: rgb"
        og += ng
        ow += nw
    share = n_close / max(n_pairs, 1)
    print(f"close share {share:.5f} of {n_pairs} (pair, pixel)s")
    if max_close is not None:
        assert share <= max_close, share
    return share


def golden_as_details(g):
    det = []
    for i, (ref, _) in enumerate(g["pairs"]):
        with np.errstate(invalid="ignore"):
            pm = (g[f"dist_{i}"] < g["kw"]["geo_pixel_thres"]) & (g[f"rel_{i}"] < np.float32(g["kw"]["geo_depth_thres"]))
        avg = np.full(g["masks"][i].shape, np.nan)
        avg[g["masks"][i]] = g[f"depth_avg_valid_{i}"]
        det.append(dict(pair_masks=pm, dist=g[f"dist_{i}"], relative_depth_diff=g[f"rel_{i}"], geo_mask_sum=g[f"geo_mask_sum_{i}"],
                        depth_est_averaged=avg))
    return det


# ------------------------------------------------------------------ GPU: the recorded reference runs
@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_fusion_equals_the_reference_on_goldens(name):
    g, want = restated(name)
    got = gpu_fuse(g["depths"], g["Ks"], g["Es"], g["colors"], g["pairs"], **g["kw"])
    # against the recorded arrays themselves (per-pair masks: the margins against the thresholds; averaged depth: where valid)
    det = golden_as_details(g)
    for i, d in enumerate(det):
        calm_pairs = ~R.close_pairs(d["dist"], d["relative_depth_diff"], g["kw"]["geo_pixel_thres"], g["kw"]["geo_depth_thres"])
        assert np.array_equal(got[3][i]["pair_masks"][calm_pairs], d["pair_masks"][calm_pairs])
        calm = calm_pairs.all(0)
        assert np.array_equal(got[3][i]["geo_mask_sum"][calm], d["geo_mask_sum"][calm])
        assert np.array_equal(got[2][i][calm], g["masks"][i][calm])
        v = calm & g["masks"][i]
        assert within_ulp(got[3][i]["depth_est_averaged"][v], d["depth_est_averaged"][v]).all()
    # ... and the full contract, clouds included, against the restatement (== the record, bit for bit, by the CPU test)
    assert np.array_equal(want[0], g["verts"]) and np.array_equal(want[1], g["vert_colors"])
    assert_fusion_matches(got, want, g["depths"], g["pairs"], g["kw"], max_close=CLOSE_SHARE)


# ------------------------------------------------------------------ GPU: order and count of the compaction
def _points_case(h, w, mode, seed):
    rng = np.random.default_rng(seed)
    mask = {"all": np.ones((h, w), bool), "none": np.zeros((h, w), bool)}.get(mode)
    if mask is None:
        mask = rng.random((h, w)) < 0.4
    avg = rng.random((h, w)) * 3 + 4
    color = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    K = np.array([[2.1 * w + 30, 0, (w - 1) / 2], [0, 2.2 * w + 30, (h - 1) / 2], [0, 0, 1.0]])
    E = np.eye(4)
    E[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    E[:3, 3] = rng.standard_normal(3)
    return mask, avg, color, K, E


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,mode", [(23, 31, "all"), (23, 31, "none"), (70, 90, "random"), (1, 1, "all"), (1, 257, "random"),
                                      (512, 512, "random"), (513, 512, "random"), (1, 262400, "random")])   # 1024, 1026, 1025 blocks
def test_points_are_the_row_major_selection(h, w, mode):
    import torch

    mask, avg, color, K, E = _points_case(h, w, mode, seed=h * 1000 + w)
    want_xyz, want_rgb = R.points(mask, avg, color, K, E)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xyz, rgb = ops.depth_points(cuda(mask.astype(np.uint8) * 255), cuda(avg), cuda(color), np.linalg.inv(K), np.linalg.inv(E))
    xyz, rgb = xyz.cpu().numpy(), rgb.cpu().numpy()
    assert xyz.shape == (int(mask.sum()), 3) and rgb.shape == xyz.shape and xyz.dtype == np.float32 and rgb.dtype == np.uint8
    assert within_ulp(xyz, want_xyz).all() and np.array_equal(rgb, want_rgb)                # index by index: the order too
    if mode == "none":                                                                      # N = 0: emit with null outputs
        lib = _lib.load()
        m, a, c = cuda(mask.astype(np.uint8)), cuda(avg), cuda(color)
        nb = lib.ufr_depth_points_workspace_bytes(h, w)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        n = C.c_int64(-1)
        s = torch.cuda.current_stream().cuda_stream
        assert lib.ufr_depth_points_count(m.data_ptr(), h, w, ws.data_ptr(), nb, C.byref(n), s) == 0 and n.value == 0
        ik, ie = (C.c_double * 9)(), (C.c_double * 16)()
        assert lib.ufr_depth_points_emit(m.data_ptr(), a.data_ptr(), c.data_ptr(), h, w, ik, ie, ws.data_ptr(), nb, None, None, 0, s) == 0
    if mode == "random" and h > 1:                                                          # a capacity below the count is refused
        lib = _lib.load()
        m, a, c = cuda(mask.astype(np.uint8)), cuda(avg), cuda(color)
        nb = lib.ufr_depth_points_workspace_bytes(h, w)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        n = C.c_int64(-1)
        s = torch.cuda.current_stream().cuda_stream
        assert lib.ufr_depth_points_count(m.data_ptr(), h, w, ws.data_ptr(), nb, C.byref(n), s) == 0 and n.value == mask.sum()
        out = torch.full((n.value, 3), 7.0, dtype=torch.float32, device="cuda")
        out8 = torch.full((n.value, 3), 7, dtype=torch.uint8, device="cuda")
        ik, ie = (C.c_double * 9)(), (C.c_double * 16)()
        assert lib.ufr_depth_points_emit(m.data_ptr(), a.data_ptr(), c.data_ptr(), h, w, ik, ie, ws.data_ptr(), nb, out.data_ptr(),
                                         out8.data_ptr(), n.value - 1, s) == -1
        assert b"capacity" in lib.ufr_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((out8 == 7).all())                         # ... and nothing was written


# ------------------------------------------------------------------ GPU: source counts, odd sizes, float32 cameras
def _odd_scene(n_src, seed):
    """a 37x53 reference view and n_src sources, alternately larger and smaller than it: the plane z = 0 seen from cameras on
    an arc, with smooth and pixel-level depth errors and holes; float32 cameras, as the model writes them"""
    rng = np.random.default_rng(seed)
    sizes = [(37, 53)] + [((61, 75) if k % 2 == 0 else (29, 41)) for k in range(n_src)]
    depths, Ks, Es, colors = [], [], [], []
    for v, (h, w) in enumerate(sizes):
        ang = 0.0 if v == 0 else 0.05 * ((v + 1) // 2) * (1 if v % 2 else -1)
        c, s = np.cos(ang), np.sin(ang)
        Rm = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        eye = np.array([-6.0 * np.sin(ang), 0.02 * v, -6.0 * np.cos(ang)])
        E = np.eye(4)
        E[:3, :3] = Rm
        E[:3, 3] = -Rm @ eye
        f = 5.0 * w
        K = np.array([[f, 0, (w - 1) / 2 + 0.3], [0, f, (h - 1) / 2 - 0.2], [0, 0, 1.0]])
        # depth of the plane z = 0 (world) seen from this camera, then errors and holes
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        rays = Rm.T @ (np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)]))
        z = (-eye[2] / rays[2]).reshape(h, w)
        z = z * (1 + 0.004 * np.sin(xs / 5.0 + v) * np.cos(ys / 4.0))
        z = z * (1 + np.where(rng.random((h, w)) < 0.3, 0.01 * rng.standard_normal((h, w)), 0))
        z[rng.random((h, w)) < 0.04] = 0
        depths.append(z.astype(np.float32))
        Ks.append(K.astype(np.float32))
        Es.append(E.astype(np.float32))
        colors.append(rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
    return depths, Ks, Es, colors


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [1, 10])
def test_source_counts_odd_sizes_and_float32_cameras(n_src):
    depths, Ks, Es, colors = _odd_scene(n_src, seed=n_src)
    pairs = [(0, list(range(1, n_src + 1)))]
    kw = dict(geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=1 if n_src == 1 else 3)
    want = R.fuse_views(depths, Ks, Es, colors, pairs, **kw)
    got = gpu_fuse(depths, Ks, Es, colors, pairs, **kw)
    assert_fusion_matches(got, want, depths, pairs, kw, max_close=CLOSE_SHARE)
    pm = want[3][0]["pair_masks"]
    assert 0.1 < pm.mean() < 0.9 and 0.05 < want[2][0].mean() < 0.95                        # the case decides something
    assert want[3][0]["geo_mask_sum"].max() >= min(n_src, 4)


# ------------------------------------------------------------------ GPU: degenerate numbers are ordinary inputs
@pytest.mark.gpu
def test_degenerate_numbers_are_inconsistent_and_harmless():
    h, w = 19, 27
    # the principal point lies between pixels: on an integer one, x of the centre column is the exact cancellation
    # 13 d / 120 - (13 / 120) d, whose fp64 residue (1e-16, fused or not) is all there is to compare
    K = np.array([[120.0, 0, 13.3], [0, 120.0, 9.4], [0, 0, 1.0]])
    flat = np.full((h, w), 5.0, np.float32)
    zero_ref = flat.copy()
    zero_ref[::2] = 0                                          # reference depth 0: relative_depth_diff is inf or NaN
    zero_ref[1, :5] = 0
    behind = np.eye(4)
    behind[:3, :3] = np.diag([-1.0, 1.0, -1.0])                # a source looking the other way: every point has z < 0
    behind[2, 3] = 2.0
    far = np.eye(4)
    far[0, 3] = 4000.0                                         # x_src = 120 * 4000 / 5 = 96000: beyond int16 after the shift
    huge = np.eye(4)
    huge[0, 3] = 1e9                                           # x_src * 32 beyond int32
    same = np.eye(4)                                           # the reference pose itself: with depth 0, K (0, 0, 0) / 0 = NaN
    depths = [zero_ref, flat, flat, flat, flat, flat]
    Ks = [K] * 6
    Es = [np.eye(4), behind, far, huge, same, np.eye(4)]
    colors = [np.zeros((h, w, 3), np.uint8)] * 6
    pairs = [(0, [1, 2, 3, 4]), (5, [1, 2, 3])]
    kw = dict(geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=1)
    want = R.fuse_views(depths, Ks, Es, colors, pairs, **kw)
    got = gpu_fuse(depths, Ks, Es, colors, pairs, **kw)
    assert_fusion_matches(got, want, depths, pairs, kw, max_close=0.0)
    pm0, pm1 = got[3][0]["pair_masks"], got[3][1]["pair_masks"]
    assert not pm0[:3].any() and not pm1.any()                                              # behind, far, huge: inconsistent
    assert not pm0[3][zero_ref == 0].any() and pm0[3][zero_ref != 0].all()                  # depth 0: inconsistent; else the same pose agrees
    assert np.array_equal(got[3][0]["geo_mask_sum"], (zero_ref != 0).astype(np.int32))
    assert len(got[0]) == int((zero_ref != 0).sum())


# ------------------------------------------------------------------ GPU: the files, end to end
@pytest.fixture(scope="module")
def depth_tree(tmp_path_factory):
    """the tree model.save_depth_outputs writes for three views of the golden scene (float32 cameras, as the model has them)"""
    from PIL import Image

    from uforecon_amd.model import save_depth_outputs

    g = load_golden("nview")
    root = str(tmp_path_factory.mktemp("fusion"))
    scan = "scan9"
    depths, Ks, Es, colors = [], [], [], []
    for v in range(3):
        K, E = g["Ks"][v].astype(np.float32), g["Es"][v].astype(np.float32)
        save_depth_outputs(root, scan, "%08d" % v, g["depths"][v], g["colors"][v].astype(np.float32) / np.float32(255), E, K)
        depths.append(g["depths"][v])
        Ks.append(K)
        Es.append(E)
        colors.append(np.array(Image.open(os.path.join(root, "rgb", scan, "%08d.jpg" % v)), dtype=np.uint8))
    pairs = [(0, [1, 2]), (1, [0, 2]), (2, [0, 1])]
    kw = dict(geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2)
    return dict(root=root, scan=scan, views=(depths, Ks, Es, colors), pairs=pairs, kw=kw,
                want=R.fuse_views(depths, Ks, Es, colors, pairs, **kw))


def _check_written_tree(t, xyz_len=None):
    from PIL import Image

    xyz_w, rgb_w, masks_w, det_w = t["want"]
    masks = []
    for i, (ref, _) in enumerate(t["pairs"]):
        png = np.array(Image.open(os.path.join(t["root"], t["scan"], "mask", "%08d.png" % ref)))
        assert png.dtype == np.uint8 and set(np.unique(png)) <= {0, 255}
        calm = ~R.close_pairs(det_w[i]["dist"], det_w[i]["relative_depth_diff"], t["kw"]["geo_pixel_thres"],
                              t["kw"]["geo_depth_thres"]).any(0)
        assert np.array_equal((png > 0)[calm], masks_w[i][calm])
        masks.append(png > 0)
    ply = os.path.join(t["root"], "pcd", t["scan"] + ".ply")
    v, f = dtu_eval.read_ply(ply)                                                           # the evaluation's reader
    assert f is None and len(v) == sum(int(m.sum()) for m in masks)
    return masks, v


@pytest.mark.gpu
def test_filter_depth_end_to_end_on_the_models_files(depth_tree, capsys):
    t = depth_tree
    xyz, rgb, masks = DF.filter_depth(t["root"], t["scan"], n_view=3)
    out = capsys.readouterr().out
    assert "processing scan9, ref-view00, geo_mask:{:3f}".format(masks[0].mean()) in out and "saving the final model to" in out
    png_masks, v = _check_written_tree(t)
    assert all(np.array_equal(a, b) for a, b in zip(png_masks, masks))
    assert np.array_equal(v, xyz.astype(np.float64))
    # the cloud against the restatement, under the contract (the details come from a second in-memory run of the same inputs)
    got = gpu_fuse(*t["views"], t["pairs"], **t["kw"])
    assert np.array_equal(got[0], xyz) and np.array_equal(got[1], rgb)                      # deterministic, and the same route
    assert_fusion_matches(got, t["want"], t["views"][0], t["pairs"], t["kw"], max_close=CLOSE_SHARE)
    assert 0.05 < np.mean([m.mean() for m in masks]) < 0.9                                  # the run decides something


@pytest.mark.gpu
def test_command_line_on_the_models_files(depth_tree):
    t = depth_tree
    ply = os.path.join(t["root"], "pcd", t["scan"] + ".ply")
    if os.path.exists(ply):
        os.rename(ply, ply + ".first")
    r = subprocess.run([sys.executable, "-m", "uforecon_amd.depth_fusion", "--root_dir", t["root"], "--n_view", "3"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "found scans: ['scan9']" in r.stdout and "processing scan9, ref-view02, geo_mask:" in r.stdout
    assert "saving the final model to " + ply in r.stdout
    _check_written_tree(t)
    if os.path.exists(ply + ".first"):                                                      # run after run, the same bytes
        assert open(ply, "rb").read() == open(ply + ".first", "rb").read()
