"""The gather's two block -> point maps (gather.hip) must be invisible in every output.

Where the sample count is a multiple of 8 and the launch has at least 8 rays, a block of gather_kernel is 8 neighbouring
rays x 8 consecutive samples (lane = ray fastest); every other shape keeps 64 consecutive points per block.  A point's
arithmetic does not depend on the block it lands in, so the same points presented as RN * SN rays of one sample each
(SN = 1: the consecutive-point map) must give the same bits in every output.  What can go wrong is the index map and its
tails only, so the shapes are small: one block, two sample groups, a 5-ray and a 1-ray tail group, a sample count that is
an odd number of groups, and a grid of more than 8 blocks (the block -> XCD remap in front of the map).
"""
import functools

import pytest
import torch

import gather_ref as G
from helpers import load_weights
from uforecon_amd import ops
from uforecon_amd.scene import make_frame, sampler_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("x", "rgb", "dir", "sim8", "vol24", "xy", "mask_z")


@pytest.fixture(scope="module")
def weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


@functools.lru_cache(maxsize=None)
def _frame(NV):
    fr = G.frame_for(NV)
    f = fr.to(DEV)
    return fr, ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)


def _gather(fh, weights, o, d, z):
    """Every output of one launch, NaN-filled beforehand: a row the kernel leaves unwritten cannot compare equal."""
    RN, SN = z.shape
    NV, P = fh.NV, RN * SN
    out = tuple(torch.full((P, NV, c), float("nan"), device=DEV) for c in (80, 4, 4))
    x, rgbm, dirs, dbg = ops.project_gather(fh, weights, o.to(DEV).contiguous(), d.to(DEV).contiguous(), z.to(DEV).contiguous(),
                                            debug=True, out=out)
    assert ops.status_poll(True) == 0
    got = dict(x=x, rgb=rgbm, dir=dirs, **dbg)
    assert sorted(got) == sorted(OUTPUTS)
    return {k: v.cpu() for k, v in got.items()}


# (RN, SN, per-ray origins)
BLOCK_SHAPES = (
    (16, 16, True),     # 2 ray groups x 2 sample groups
    (13, 24, True),     # a 5-ray tail group, 3 sample groups
    (8, 8, False),      # one block
    (9, 64, False),     # a 1-ray tail group; 16 blocks: the first 16 go through the block -> XCD remap
    (21, 40, True),     # 15 blocks: 8 remapped, 7 not; 5 sample groups
)


@pytest.mark.parametrize("RN,SN,per_ray", BLOCK_SHAPES)
@pytest.mark.parametrize("NV", (3, 5))
def test_ray_blocks_equal_single_sample_rays(NV, RN, SN, per_ray, weights):
    fr, fh = _frame(NV)
    o, d, z = G.offaxis_rays(fr, RN, SN, NV, per_ray)
    assert SN % 8 == 0 and RN >= 8                                    # the ray-block map
    blocks = _gather(fh, weights, o, d, z)
    o1 = o.repeat_interleave(SN, 0) if per_ray else o
    points = _gather(fh, weights, o1, d.repeat_interleave(SN, 0), z.reshape(-1, 1))     # SN = 1: 64 consecutive points
    for k in OUTPUTS:
        assert not bool(torch.isnan(blocks[k]).any()), (k, "unwritten rows")
        assert torch.equal(blocks[k], points[k]), k


def test_other_sample_counts_keep_the_point_map(weights):
    """SN = 12 is no multiple of 8: 64 consecutive points per block, compared with the float64 rows under the bounds of
    tests/test_gpu_gather.py (yardstick = the fp32 oracle's own distance from float64, on this set and on the pool set)."""
    NV, RN, SN = 3, 11, 12
    fr, fh = _frame(NV)
    P = load_weights()
    o, d, z = G.offaxis_rays(fr, RN, SN, NV, True)
    r64, r32 = G.rows(P, fr, o, d, z), G.rows(P, fr, o, d, z, torch.float32)
    po, pd, pz = G.offaxis_rays(fr, *G.POOL_SHAPE[:2], NV, G.POOL_SHAPE[2])
    pool = G.row_errors(G.rows(P, fr, po, pd, pz, torch.float32), G.rows(P, fr, po, pd, pz))
    yard = G.yardstick(G.row_errors(r32, r64), pool)
    g = _gather(fh, weights, o, d, z)
    got = dict(x=g["x"], rgb=g["rgb"][..., :3], dirs=g["dir"][..., :3], xy=g["xy"].reshape(NV, RN, SN, 2),
               sim8=g["sim8"].reshape(RN, SN, 8), vol24=g["vol24"].reshape(RN, SN, 24))
    err = G.row_errors(got, r64)
    for k in ("xy", "sim8", "vol24", "feat", "vol", "sim16", "rgb", "dirs"):
        b = G.bound(yard[k], G.ROW_CAPS[k])
        print(f"GATHER SN=12 {k}: kernel {err[k]:.2e} yardstick {yard[k]:.2e} bound {b:.2e}")
        assert err[k] < b, (k, err[k], b)
    pe = g["x"][..., 72:80].double().reshape(RN, SN, NV, 8).permute(2, 0, 1, 3)
    pe64 = r64["x"][..., 72:80].reshape(RN, SN, NV, 8).permute(2, 0, 1, 3)
    assert float(((pe - pe64).abs() / G.pe_tolerance(fr, r32, r64)).max()) <= 1.0
    cmp = G.comparable(r64)
    assert torch.equal(g["mask_z"].reshape(NV, RN, SN).double()[cmp], r64["mask_z"][cmp])
    assert torch.equal(g["rgb"][..., 3].reshape(RN, SN, NV).permute(2, 0, 1).double()[cmp], r64["mask"][cmp])
    # ... and the same points one by one, bit for bit
    points = _gather(fh, weights, o.repeat_interleave(SN, 0), d.repeat_interleave(SN, 0), z.reshape(-1, 1))
    for k in OUTPUTS:
        assert torch.equal(g[k], points[k]), k


@pytest.mark.parametrize("RN", (40, 43))
def test_render_rays_ray_tails_inside_chunks(RN, weights):
    """The whole path, 16 + 16 samples: chunks of 16 rays (whole ray groups, and at RN = 43 an 11-ray last chunk with a
    3-ray tail group) against one chunk of all rays (RN = 43: a 3-ray tail group in another place), coarse pass and
    fine-pass pool, bit for bit."""
    fr = make_frame(64, 96, 3, seed=0)
    f = fr.to(DEV)
    fh = ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)
    idx = (torch.arange(RN) * 131 + 300).to(DEV)
    U1, U2 = (u.to(DEV) for u in sampler_uniforms(4, 16, 16, RN))
    a = ops.render_rays(fh, weights, idx, U1, U2, workspace=ops.RenderWorkspace(DEV, 16, 16, 3, chunk_rays=16))
    a = {k: v.clone() for k, v in a.items() if torch.is_tensor(v)}
    b = ops.render_rays(fh, weights, idx, U1, U2, workspace=ops.RenderWorkspace(DEV, 16, 16, 3, chunk_rays=RN))
    assert ops.status_poll(True) == 0
    for k in ("depth", "depth_z", "rgb", "srdf", "z_all"):
        assert not bool(torch.isnan(a[k]).any()), k
        assert torch.equal(a[k], b[k]), k
