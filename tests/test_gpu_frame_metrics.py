"""ufr_frame_metrics / ufr_frame_preview_u8 (csrc/frame_metrics.hip) against the float64 forms of tests/frame_metrics_ref.py
and against torch's own fp32 losses.

Bounds.  Every summand of the six scores is >= 0, so a double sum taken in another order is off by at most (n - 1) 2^-53
relative: 1e-9 holds for every n here; the count and the max are exact.  torch's fp32 `mse_loss` / `l1_loss` on the CPU carry
up to 3n 2^-24 relative error of their own (the bound of an fp32 sum of 3n non-negative terms), which is what the kernel is
allowed to differ from them by."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_metrics_ref as R
from uforecon_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR, FAR = 2.25, 3.75      # exact in float32
GRID = 256 * 256            # threads of the largest grid (csrc/frame_metrics.hip): n above it runs the stride loop twice
SIZES = [1, 63, 64, 65, 256 * 3 + 1, 48 * 64, GRID + 4097]


def make_case(n, seed=0, valid="some"):
    g = torch.Generator().manual_seed(1000 + seed + n)
    c = dict(rgb_c=torch.rand(n, 3, generator=g) * 1.6 - 0.3,        # colours outside [0,1]: PSNR clamps, MSE does not
             rgb_f=torch.rand(n, 3, generator=g) * 1.6 - 0.3,
             rgb_gt=torch.rand(3, n, generator=g) * 1.2 - 0.1,
             depth_c=2.0 + 2.0 * torch.rand(n, generator=g),
             depth_f=2.0 + 2.0 * torch.rand(n, generator=g))
    gt = 1.5 + 3.0 * torch.rand(n, generator=g)                       # some below near, some above far
    if valid == "some":
        gt[torch.rand(n, generator=g) < 0.2] = 0.0                    # holes
        if n >= 4:
            gt[0], gt[1], gt[2], gt[3] = NEAR, FAR, 0.0, 3.0          # both ends are inside the mask; 0 is a hole
    elif valid == "none":
        gt = torch.where(torch.rand(n, generator=g) < 0.5, torch.zeros(n), torch.full((n,), FAR + 1.0))
    c["depth_gt"] = gt
    return c


def run(c):
    d = {k: v.to(DEV).contiguous() for k, v in c.items()}
    out = ops.frame_metrics(d["rgb_c"], d["rgb_f"], d["rgb_gt"], d["depth_c"], d["depth_f"], d["depth_gt"], NEAR, FAR)
    return out.cpu().numpy()


def ref(c):
    return R.frame_metrics(c["rgb_c"], c["rgb_f"], c["rgb_gt"], c["depth_c"], c["depth_f"], c["depth_gt"], NEAR, FAR)


@pytest.mark.parametrize("n", SIZES)
def test_against_float64(n):
    c = make_case(n)
    got, want = run(c), ref(c)
    print(n, got, want)
    for i in range(6):
        assert abs(got[i] - want[i]) <= 1e-9 * abs(want[i]), (i, got[i], want[i])
    assert got[6] == want[6] and got[7] == want[7]
    if n >= 4:
        assert want[6] >= 2            # the pixels at near and at far count


@pytest.mark.parametrize("n", SIZES)
def test_against_torch_fp32(n):
    c = make_case(n, seed=5)
    got = run(c)
    gt = c["rgb_gt"].t()
    bound = 3 * n * 2.0 ** -24
    for i, x in ((0, c["rgb_c"]), (1, c["rgb_f"])):
        t = float(F.mse_loss(x, gt))
        assert abs(got[i] - t) <= bound * abs(t) + 1e-12, (i, got[i], t)
    m = (c["depth_gt"] != 0) & (c["depth_gt"] >= NEAR) & (c["depth_gt"] <= FAR)
    if int(m.sum()):
        for i, d in ((4, c["depth_c"]), (5, c["depth_f"])):
            t = float(F.l1_loss(d[m], c["depth_gt"][m]))
            assert abs(got[i] - t) <= bound * abs(t) + 1e-12, (i, got[i], t)
    else:
        assert got[4] == 0.0 and got[5] == 0.0
    assert got[6] == float(m.sum())


@pytest.mark.parametrize("n", [65, 48 * 64])
def test_no_valid_pixel(n):
    got = run(make_case(n, valid="none"))
    assert got[4] == 0.0 and got[5] == 0.0 and got[6] == 0.0


def test_mask_edges():
    """near and far themselves are valid, 0 and the values just outside are not."""
    n = 6
    c = make_case(n, valid="all")
    below, above = np.nextafter(np.float32(NEAR), np.float32(0)), np.nextafter(np.float32(FAR), np.float32(9))
    c["depth_gt"] = torch.tensor([NEAR, FAR, 0.0, float(below), float(above), 3.0])
    got, want = run(c), ref(c)
    assert got[6] == 3.0 == want[6]
    d = (c["depth_c"].double() - c["depth_gt"].double()).abs()
    assert abs(got[4] - float((d[0] + d[1] + d[5]) / 3)) <= 1e-12


def test_clamp_matters_for_psnr_only():
    n = 256 * 3 + 1
    c = make_case(n, seed=2)
    got = run(c)
    clamped = dict(c, rgb_c=c["rgb_c"].clamp(0, 1), rgb_f=c["rgb_f"].clamp(0, 1), rgb_gt=c["rgb_gt"].clamp(0, 1))
    got_k = run(clamped)
    assert got[2] == got_k[2] and got[3] == got_k[3]        # PSNR sees the clamped colours either way
    assert got[0] != got_k[0] and got[1] != got_k[1]        # MSE does not clamp


def test_nan_depth_reaches_l1_and_leaves_mse():
    n = 48 * 64
    c = make_case(n, seed=3)
    clean = run(c)
    c["depth_gt"][100] = 3.0
    c["depth_f"][100] = float("nan")
    got = run(c)
    assert np.isnan(got[5]) and not np.isnan(got[4])
    assert got[0] == clean[0] and got[1] == clean[1] and got[2] == clean[2] and got[3] == clean[3]
    c["depth_c"][7] = float("nan")
    assert np.isnan(run(c)[7])                               # np.max propagates NaN
    c = make_case(n, seed=3)
    c["depth_gt"][5] = float("nan")                          # a NaN ground truth fails the mask, as in torch
    assert not np.isnan(run(c)[4:6]).any()


@pytest.mark.parametrize("n", [48 * 64, GRID + 4097])
def test_rerun_gives_the_same_bits(n):
    c = make_case(n, seed=4)
    a, b = run(c), run(c)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [1, 65, 48 * 64])
def test_preview_bytes_equal_numpy(n):
    g = torch.Generator().manual_seed(77 + n)
    rgb = torch.rand(n, 3, generator=g)
    # values whose product with 255 lies within one ulp of an integer, on both sides
    k = torch.arange(0, 256, dtype=torch.float32)
    exact = (k / 255).numpy().astype(np.float32)
    edge = np.concatenate([exact, np.nextafter(exact, np.float32(2)), np.nextafter(exact, np.float32(-1))]).clip(0, 1)
    m = min(edge.size, rgb.numel())
    rgb.view(-1)[:m] = torch.from_numpy(edge[:m])
    depth = 2.0 + 2.0 * torch.rand(n, generator=g)
    if n > 3:
        depth[1] = depth.max()                                # the quotient 1.0 itself -> 255
        depth[2] = float(np.nextafter(np.float32(depth.max()), np.float32(0)))
    scale = 1.7320508
    dmax = depth.max().double().reshape(1).to(DEV)
    rgb8, depth8 = ops.frame_preview_u8(rgb.to(DEV), depth.to(DEV), dmax, scale)
    want_rgb, want_depth = R.preview_u8(rgb, depth, scale)
    assert np.array_equal(rgb8.cpu().numpy(), want_rgb)
    assert np.array_equal(depth8.cpu().numpy(), want_depth)
    only_rgb, none = ops.frame_preview_u8(rgb.to(DEV))
    assert none is None and np.array_equal(only_rgb.cpu().numpy(), want_rgb)


def test_argument_errors():
    lib = _lib.load()
    t = torch.zeros(8, device=DEV)
    o = torch.zeros(8, dtype=torch.float64, device=DEV)
    p, q = t.data_ptr(), o.data_ptr()
    assert lib.ufr_frame_metrics(p, p, p, p, p, p, 0.0, 1.0, 0, q, q, None) == -1
    assert lib.ufr_frame_metrics(p, p, None, p, p, p, 0.0, 1.0, 1, q, q, None) == -1
    assert lib.ufr_frame_metrics(p, p, p, p, p, p, 0.0, 1.0, 1, None, q, None) == -1
    assert lib.ufr_frame_metrics(p, p, p, p, p, p, 0.0, 1.0, 2 ** 30, q, q, None) == -1
    assert lib.ufr_frame_preview_u8(p, None, None, 1.0, 1, None, None, None) == -1       # rgb without rgb8
    assert lib.ufr_frame_preview_u8(None, p, None, 1.0, 1, None, p, None) == -1          # depth without its max
    assert lib.ufr_frame_preview_u8(None, p, q, 0.0, 1, None, p, None) == -1             # scale must be > 0
    assert lib.ufr_frame_preview_u8(None, None, None, 1.0, 1, None, None, None) == -1
    assert lib.ufr_frame_metrics_workspace_bytes(1) >= 256 * 8 * 8
