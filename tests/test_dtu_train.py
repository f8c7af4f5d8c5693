"""uforecon_amd.dtu_train.DtuTrain(device="cpu") against the reference's own MVSDataset, recorded in
tests/golden/dtu_train_small.npz by tests/golden/make_golden_dtu_train.py (keys, shapes, dtypes, meta, values)."""
import numpy as np
import pytest

import dtu_train_golden as G
from dtu_scan_golden import TOL_ULPS as SCAN_TOL
from uforecon_amd._lib import UfrError

# the bounds tests/test_dtu_scan.py uses for the same quantities (tests/dtu_scan_golden.py: float32 steps at the key's largest
# magnitude, for entries that went through LAPACK / BLAS); c2ws is the inverse pair of w2cs, trans_mat an inverse like ref_pose_inv
TOL_ULPS = dict(SCAN_TOL, c2ws=SCAN_TOL["w2cs"], trans_mat=SCAN_TOL["ref_pose_inv"], cam_ray_d=SCAN_TOL["ray_d"])
FLOAT64_IN_THE_REFERENCE = ("ray_d", "cam_ray_d", "depths_h")      # returned as float32 here (uforecon_amd/dtu_train.py)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return G.write_tree(tmp_path_factory.mktemp("dtu_train"))


@pytest.fixture(scope="module")
def datasets(tree):
    return {case: G.open_dataset(tree, case, "cpu") for case in G.cases()}


def _close(got, want, key):
    if key not in TOL_ULPS:
        return np.array_equal(got, want)
    step = float(np.spacing(np.float32(np.abs(want).max())))
    return float(np.abs(got.astype(np.float64) - want).max()) <= TOL_ULPS[key] * step


@pytest.mark.parametrize("case,i", [(c, i) for c, ii in G.items().items() for i in ii])
def test_item_is_the_references(datasets, case, i):
    want = G.golden_item(case, i)
    got = G.flat_batch(datasets[case][i])
    keys = {k.split(".")[0] if k.split(".")[0] in ("images", "ref_img", "source_imgs") + FLOAT64_IN_THE_REFERENCE else k for k in want}
    assert set(got) == keys, set(got) ^ keys
    assert got["meta"] == want["meta"]
    for k in ("images", "ref_img", "source_imgs") + FLOAT64_IN_THE_REFERENCE:          # recorded as shape and dtype (+ a pixel set)
        assert got[k].shape == tuple(want[k + ".shape"]), k
        ref_dtype = str(want[k + ".dtype"])
        assert ref_dtype == ("float64" if k in FLOAT64_IN_THE_REFERENCE else "float32") and got[k].dtype == np.float32, k
    assert np.array_equal(got["ref_img"], got["images"][:, 0]) and np.array_equal(got["source_imgs"], got["images"][:, 1:])
    for k, w in want.items():
        if k == "meta" or k.endswith((".shape", ".dtype")) or k.split(".")[0] in G.PIXEL_KEYS:
            continue
        assert got[k].shape == w.shape and got[k].dtype == w.dtype, (k, got[k].shape, got[k].dtype, w.shape, w.dtype)
        assert _close(got[k], w, k.split(".")[0]), k
    if "images" not in want:
        return
    assert np.array_equal(G.at_pixels(got["images"], 3), want["images"].astype(np.float32) / np.float32(255))
    for k in ("ray_d", "cam_ray_d"):
        assert _close(G.at_pixels(got[k], 2), want[k], k), k
    d, dw = G.at_pixels(got["depths_h"], 2), want["depths_h"]
    assert np.array_equal(d == 0, dw == 0) and (dw == 0).any() and (dw != 0).any()              # the holes, exactly
    nf = want["near_fars"][0, 0]
    assert (dw[dw != 0] < nf[0]).any() or (dw > nf[1]).any()                                     # values outside near / far exist
    if np.array_equal(got["scale_factor"], want["scale_factor"]) and np.array_equal(G.at_pixels(got["cam_ray_d"], 2), want["cam_ray_d"]):
        assert np.array_equal(d, dw)                                                             # bit for bit
    else:       # another machine's LAPACK moved scale_factor / cam_ray_d by a few steps: the depths follow them
        assert np.abs(d.astype(np.float64) - dw).max() <= (TOL_ULPS["scale_factor"] + TOL_ULPS["cam_ray_d"] + 1) * np.spacing(np.float32(np.abs(dw).max()))


@pytest.mark.parametrize("case", list(G.cases()))
def test_len_and_meta_order(datasets, case):
    ds = datasets[case]
    assert len(ds) == int(G.golden()[f"{case}/len"])
    assert [(m[0], m[1], m[2], list(m[3])) for m in ds.metas] == [(m[0], m[1], m[2], list(m[3])) for m in G.metas(case)]


def test_last_camera_file_sets_the_depth_range(datasets):
    ds = datasets["test"]
    assert ds.depth_min == 425.0 + 0.25 * (48 % 5) and ds.depth_interval == 2.5 * 1.06


def test_random_selection_is_reproducible_under_seed(tree):
    a = G.open_dataset(tree, "train", "cpu", view_selection_type="random", seed=5)
    b = G.open_dataset(tree, "train", "cpu", view_selection_type="random", seed=5)
    c = G.open_dataset(tree, "train", "cpu", view_selection_type="random", seed=6)
    assert a.metas == b.metas and a.metas != c.metas
    assert all(len(m[3]) == 4 and m[2] not in m[3] and len(set(m[3])) == 4 for m in a.metas)


def test_too_many_source_views_is_one_line(tree):
    with pytest.raises(UfrError) as e:
        G.open_dataset(tree, "test", "cpu", test_ref_views=list(range(20, 29)))
    assert "\n" not in str(e.value) and "UFR_MAX_VIEWS" in str(e.value)


def test_depth_host_form_is_the_float64_reference():
    """depth_gt_host against tests/frame_metrics_ref.read_depth's float32 chain: equal where the divisor is a float32 value."""
    import frame_metrics_ref as R
    from uforecon_amd.dtu_train import depth_gt_host

    rng = np.random.default_rng(3)
    rows = rng.uniform(300, 900, (25, 41)).astype(np.float32)
    rows[rng.uniform(size=rows.shape) < 0.2] = 0.0
    z = rng.uniform(0.9, 1.0, 8 * 12).astype(np.float32)
    for bottom_up in (True, False):
        got = depth_gt_host(rows, bottom_up, 2, 3, 8, 12, 0.0017, z.astype(np.float64))
        flipped = np.flipud(rows) if bottom_up else rows
        scaled = flipped[0::2, 0::2][2:10, 3:15] * np.float32(0.0017)
        want = (scaled.astype(np.float64).reshape(-1) / z.astype(np.float64)).astype(np.float32).reshape(8, 12)
        assert np.array_equal(got, want) and np.array_equal(got == 0, scaled == 0)
        # the all-float32 chain differs from it by at most one float32 step (one more rounding)
        f32 = R.read_depth(rows, bottom_up, 2, 3, 8, 12, 0.0017, z)
        assert np.abs(got.astype(np.float64) - f32).max() <= np.spacing(np.float32(np.abs(f32).max()))
