"""The forward of the view and ray transformers (with the SRDF and radiance heads) against the oracle in float64.

Tokens come from the HIP gather on a seeded 48 x 64 training-layout frame per view count, as in the backward tests; both
sides see the same float32 inputs.  Two metrics per tensor (tests/forward_ref.py): the whole-tensor helpers.rel_err and the
worst ROW (a token's 80 / 88 channels, a point's colour with the RGB floor 0.05, a ray's SRDF), which shows an error
confined to one token slot or one padding column at its own size.

fp32 mode: the row bounds of test_aggregate_rows (2e-5; srdf 5e-5), each at least twice the float32 oracle's own distance
from float64 on the same case (tests/test_forward_refs.py keeps that below 2e-6, so the project's bounds are what holds).
  (a) ufr_aggregate at every view count x ray-tile class x forced masks,
  (b) ufr_view_transform at every point count 1..45 of every instantiation,
  (c) its second grid iteration (90 000 points),
  (d) the 16-bit matrix mode on the grid of (a): bounds measured on the MI355X, written beside their constants.
"""
import functools

import pytest
import torch

import forward_ref as F
from helpers import load_weights
from uforecon_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32, LOWP = ops.PRECISION_FP32, ops.PRECISION_16BIT
NVS = [2, 3, 4, 5, 6, 7]
BLEND_OF_MASKED = 2e-5      # a point whose views are all masked: its colour against the plain mean of the views' colours

# 16-bit mode (one fp16 plane per operand), (whole tensor, worst row) against float64: no bound can be derived for it, so
# each is 2 x the worst value measured on the MI355X over AGG_SHAPES with gathered masks (the kernels are deterministic:
# the factor covers the input dependence of fp16 rounding alone).  Measured worst, and the case that gave it:
MEASURED16 = dict(
    view_out=(6.43e-4, 1.22e-3),    # NV 3, SN 48, RN 3 / NV 7, SN 32, RN 4
    ray_out=(6.69e-4, 1.00e-3),     # NV 4, SN 80, RN 3 (both)
    radiance=(5.28e-5, 8.29e-5),    # NV 4, SN 80, RN 3 / NV 7, SN 32, RN 4
    srdf=(1.27e-3, 1.43e-3),        # NV 4, SN 80, RN 3 (both)
)
FURTHER16 = 10.0            # 16-bit mode's worst tensor is at least this many times fp32 mode's on the same case


@functools.lru_cache(maxsize=None)
def _weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


@functools.lru_cache(maxsize=None)
def _frame_handle(NV):
    f = F.frame(NV).to(DEV)
    return ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)


@functools.lru_cache(maxsize=4)
def _gathered(NV, RN, SN, seed):
    """(x (P,NV,80), rgbm (P,NV,4), dirs (P,NV,4)) of RN rays x SN samples of frame(NV), through the HIP gather"""
    ray_o, ray_d, near, far, U = (t.to(DEV) for t in F.ray_inputs(NV, RN, SN, seed))
    z = ops.sample_fixed(near, far, U)
    x, rgbm, dirs, _ = ops.project_gather(_frame_handle(NV), _weights(), ray_o, ray_d, z)
    return x, rgbm, dirs


def _worst_rows(got, ref, floor, n=5):
    e = F.row_errs(got, ref, floor)
    top = torch.argsort(e, descending=True)[:n]
    return [(int(i), float(e[i])) for i in top]


def _check(label, got, ref64, ref32, bounds=None):
    """Both metrics of every tensor of ``ref64`` within its bound.  -> {name: (whole, row)}"""
    e, y = F.errors(got, ref64), F.errors(ref32, ref64)
    print(f"MEASURE {label}: " + "  ".join(f"{k} {e[k][0]:.2e}/{e[k][1]:.2e} (float32 oracle {y[k][0]:.1e}/{y[k][1]:.1e})" for k in e))
    for k, (whole, row) in e.items():
        b = bounds[k] if bounds else (F.ROW_BOUNDS[k], F.ROW_BOUNDS[k])
        assert whole < F.bound(b[0], y[k][0]), (label, k, whole)
        assert row < F.bound(b[1], y[k][1]), (label, k, row, "rows", _worst_rows(got[k], ref64[k], F.ROW_FLOORS.get(k, 1e-30)))
    return e


def _aggregate(x, rgbm, dirs, RN, SN, precision=None):
    radiance, srdf, dbg = ops.aggregate(_weights(), x, rgbm, dirs, RN, SN, debug=True, precision=precision)
    assert ops.status_poll(True) == 0
    return dict(view_out=dbg["view_out"].cpu(), ray_out=dbg["ray_out"].cpu(), radiance=radiance.cpu(), srdf=srdf.cpu())


# ------------------------------------------------------------------ (a) the aggregate grid
@pytest.mark.parametrize("masks", F.MASKS)
@pytest.mark.parametrize("NV,SN,RN", F.AGG_SHAPES)
def test_aggregate_rows_against_float64(NV, SN, RN, masks):
    x, rgbm, dirs = _gathered(NV, RN, SN, NV)
    rgbm = rgbm.clone()
    pts = F.force_masks(rgbm, masks)
    got = _aggregate(x, rgbm, dirs, RN, SN, FP32)
    xc, mc, dc = x.cpu(), rgbm.cpu(), dirs.cpu()
    _check(f"aggregate NV={NV} SN={SN} RN={RN} {masks}", got, F.aggregate_ref(xc, mc, dc, RN, SN),
           F.aggregate_ref(xc, mc, dc, RN, SN, torch.float32))
    if masks == "all_masked":
        # the -1e9 logits of such a point are all equal (torch.where): a uniform blend, whatever the logits were
        p = pts.cpu()
        mean = mc[p, :, :3].double().mean(1)
        assert F.row_err(got["radiance"][p], mean, F.RGB_FLOOR) < BLEND_OF_MASKED


# ------------------------------------------------------------------ (b) every point count
def _points(NV):
    """POINTS points of tokens, masks alternating through gathered / all masked / one view left"""
    x, rgbm, dirs = (t[:F.POINTS].clone() for t in _gathered(NV, 3, 16, 50 + NV))
    F.alternate_masks(rgbm)
    return x, rgbm, dirs


def _view(x, rgbm, dirs, precision=FP32):
    token0, radiance = ops.view_transform(_weights(), x, rgbm, dirs, precision=precision)
    return dict(token0=token0, radiance=radiance)


@pytest.mark.parametrize("NV", NVS)
def test_view_transform_at_every_point_count(NV):
    """P = 1..45 crosses every partial column tile, wave and workgroup boundary of every instantiation (16 // (NV + 1)
    points per tile) without knowing the tile constants.  Rows [:p] of the call with p points are the float64 rows within
    the bound AND the bits of the call with all 45 points."""
    x, rgbm, dirs = _points(NV)
    ref64, ref32 = F.view_ref(x.cpu(), rgbm.cpu(), dirs.cpu()), F.view_ref(x.cpu(), rgbm.cpu(), dirs.cpu(), torch.float32)
    full = _view(x, rgbm, dirs)
    parts = [_view(x[:p], rgbm[:p], dirs[:p]) for p in range(1, F.POINTS + 1)]
    assert ops.status_poll(True) == 0
    worst = {k: [0.0, 0.0] for k in ref64}
    for p, part in enumerate(parts, 1):
        for k in ref64:
            assert tuple(part[k].shape) == (p,) + tuple(ref64[k].shape[1:])
            assert torch.equal(part[k], full[k][:p]), (NV, p, k)
        e = F.errors({k: v.cpu() for k, v in part.items()}, {k: v[:p] for k, v in ref64.items()})
        y = F.errors({k: v[:p] for k, v in ref32.items()}, {k: v[:p] for k, v in ref64.items()})
        for k, (whole, row) in e.items():
            worst[k] = [max(worst[k][0], whole), max(worst[k][1], row)]
            b = F.ROW_BOUNDS["view_out" if k == "token0" else k]
            assert whole < F.bound(b, y[k][0]) and row < F.bound(b, y[k][1]), (NV, p, k, whole, row)
    y = F.errors(ref32, ref64)
    print(f"MEASURE view NV={NV} P=1..{F.POINTS}: " + "  ".join(
        f"{k} {worst[k][0]:.2e}/{worst[k][1]:.2e} (float32 oracle at P={F.POINTS} {y[k][0]:.1e}/{y[k][1]:.1e})" for k in worst))


# ------------------------------------------------------------------ (c) the second grid iteration
BIG_P, SLICE_P = 90_000, 30_011     # above 8192 waves x 10 points: more than one grid iteration at every NV, a ragged last one


@pytest.mark.parametrize("NV", NVS)
def test_view_transform_second_grid_iteration(NV):
    """One launch over 90 000 points equals, bit for bit, the same rows computed in slices of 30 011 points (each a single
    grid iteration, and every point at another position of its tile); its first and last 45 rows meet the float64 bound."""
    x45, rgbm45, dirs45 = _points(NV)
    reps = BIG_P // F.POINTS
    scale = torch.linspace(0.5, 1.5, reps, device=DEV)          # rows differ from repeat to repeat
    x = (x45[None] * scale[:, None, None, None]).reshape(BIG_P, NV, 80).contiguous()
    rgbm, dirs = rgbm45.repeat(reps, 1, 1), dirs45.repeat(reps, 1, 1)
    one = _view(x, rgbm, dirs)
    cuts = list(range(0, BIG_P, SLICE_P)) + [BIG_P]
    sliced = [_view(x[a:b], rgbm[a:b], dirs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert ops.status_poll(True) == 0
    for k in one:
        assert torch.equal(one[k], torch.cat([s[k] for s in sliced])), (NV, k)
    ends = torch.cat([torch.arange(F.POINTS), torch.arange(BIG_P - F.POINTS, BIG_P)]).to(DEV)
    xe, me, de = x[ends].cpu(), rgbm[ends].cpu(), dirs[ends].cpu()
    e = _check(f"view NV={NV} P={BIG_P} first and last {F.POINTS} rows", {k: v[ends].cpu() for k, v in one.items()},
               F.view_ref(xe, me, de), F.view_ref(xe, me, de, torch.float32),
               bounds=dict(token0=(F.ROW_BOUNDS["view_out"],) * 2, radiance=(F.ROW_BOUNDS["radiance"],) * 2))
    assert set(e) == {"token0", "radiance"}


# ------------------------------------------------------------------ (d) the 16-bit matrix mode
@pytest.mark.parametrize("NV,SN,RN", F.AGG_SHAPES)
def test_aggregate_rows_16bit_matrix_mode(NV, SN, RN):
    """precision = UFR_PRECISION_16BIT on the grid of (a): within the measured bounds of float64, at least FURTHER16 times
    further from it than fp32 mode (the mode applied), and the default mode afterwards gives the bits it gave before."""
    x, rgbm, dirs = _gathered(NV, RN, SN, NV)
    xc, mc, dc = x.cpu(), rgbm.cpu(), dirs.cpu()
    ref64, ref32 = F.aggregate_ref(xc, mc, dc, RN, SN), F.aggregate_ref(xc, mc, dc, RN, SN, torch.float32)
    before = _aggregate(x, rgbm, dirs, RN, SN)
    low = _aggregate(x, rgbm, dirs, RN, SN, LOWP)
    after = _aggregate(x, rgbm, dirs, RN, SN)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    e32 = F.errors(before, ref64)
    e16 = _check(f"16-bit aggregate NV={NV} SN={SN} RN={RN}", low, ref64, ref32,
                 bounds={k: tuple(2.0 * v for v in m) for k, m in MEASURED16.items()})
    w32, w16 = max(v[0] for v in e32.values()), max(v[0] for v in e16.values())
    assert w16 > FURTHER16 * max(w32, 1e-7), (w16, w32)
