"""The forward-only ray transformer walks sweep 1 over PAIRS of 16-token column tiles (one weight pass per pair, head
group by head group: csrc/ray_transformer.hip); the tape instantiation keeps one tile per pass in the blob's order.  Both
are documented to run the same arithmetic, so ufr_ray_transform_tape is the in-tree comparator here.

Shapes (RN, SN): (5, 16) one tile -- a pass with a dead partner; (5, 32) one full pair; (5, 48) pair + single; (3, 128) the
workload's fine length; (1, 240) 15 tiles.  RN = 5 leaves a partial 4-ray workgroup.  Each shape runs in slot order
(row=None) and through a row table that draws the RN x SN slots from a pool of 2 x RN x SN rows in shuffled order, in both
matrix precisions.  Weights: the seed-0 random initialisation; tokens: the oracle's gather of tests/forward_ref.py through
the HIP view transformer (float32), which both sides of every comparison read.

  (a) srdf equals, bit for bit, what ufr_ray_transform_tape returns for the same inputs,
  (b) srdf is within the float64 oracle's bound.  fp32 mode: forward_ref.ROW_BOUNDS["srdf"] (5e-5, worst ray).  The 16-bit
      mode runs one fp16 plane per operand and sits at 1e-3 by construction -- ROW_BOUNDS is the fp32 mode's bound -- so it
      is held to the project's own 16-bit bound, 2 x test_gpu_forward_rows.MEASURED16["srdf"], and (a) ties it to the
      tape build bit for bit,
  (c) each ray's row equals, bit for bit, the same ray run alone (RN = 1),
  (d) the sticky range status stays clear,
  (e) one NaN token raises the same status bits as in the tape build, and the other rays keep their bits.
"""
import functools

import pytest
import torch

import bwd_ref as R
import forward_ref as F
from helpers import load_weights
from test_gpu_forward_rows import MEASURED16
from uforecon_amd import ops
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32, LOWP = ops.PRECISION_FP32, ops.PRECISION_16BIT
NV = 3
SHAPES = [(5, 16), (5, 32), (5, 48), (3, 128), (1, 240)]
SRDF_BOUND = {FP32: F.ROW_BOUNDS["srdf"], LOWP: 2.0 * MEASURED16["srdf"][1]}


@functools.lru_cache(maxsize=None)
def _weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


@functools.lru_cache(maxsize=None)
def _case(RN, SN):
    """(token0 (RN*SN,80) on the GPU, float64 srdf (RN,SN) of exactly those tokens): computed once, shared, left unchanged"""
    x, rgbm, dirs = (t.to(DEV) for t in F.oracle_tokens(NV, RN, SN, 7 + SN))
    token0, _ = ops.view_transform(_weights(), x, rgbm, dirs, precision=FP32)
    P64 = {k: v.double() for k, v in load_weights().items()}
    with torch.no_grad():
        ref = R.ray_stage(P64, token0.cpu().double(), RN, SN)
    return token0, ref


def _pooled(token0, RN, SN):
    """(pool (2 RN SN, 80), row (RN,SN) int32): the slots' tokens scattered over a pool twice their number"""
    g = torch.Generator().manual_seed(1000 + 17 * SN + RN)
    M = 2 * RN * SN
    row = torch.randperm(M, generator=g)[:RN * SN]
    pool = (torch.rand(M, 80, generator=g) - 0.5).to(DEV)       # rows no slot names: never read
    pool[row.to(DEV)] = token0
    return pool, row.reshape(RN, SN).to(torch.int32).to(DEV)


def _inputs(RN, SN, pooled):
    token0, ref = _case(RN, SN)
    if pooled:
        pool, row = _pooled(token0, RN, SN)
        return pool, row, ref
    return token0, None, ref


def _tape(tok, RN, SN, row, precision):
    return ops.ray_transform_tape(_weights(), tok, RN, SN, ops.ray_transform_bwd_workspace(RN, SN, DEV), row=row, precision=precision)


def _alone(tok, SN, row, r, precision):
    """ray r of the launch, run with RN = 1"""
    if row is None:
        return ops.ray_transform(_weights(), tok[r * SN:(r + 1) * SN].contiguous(), 1, SN, precision=precision)
    return ops.ray_transform(_weights(), tok, 1, SN, row=row[r:r + 1].contiguous(), precision=precision)


@pytest.mark.parametrize("precision", [FP32, LOWP], ids=["fp32", "16bit"])
@pytest.mark.parametrize("pooled", [False, True], ids=["slots", "rows"])
@pytest.mark.parametrize("RN,SN", SHAPES)
def test_ray_pairs(RN, SN, pooled, precision):
    tok, row, ref = _inputs(RN, SN, pooled)
    assert ops.status_poll(True) == 0
    srdf = ops.ray_transform(_weights(), tok, RN, SN, row=row, precision=precision)
    tape = _tape(tok, RN, SN, row, precision)
    alone = torch.cat([_alone(tok, SN, row, r, precision) for r in range(RN)])
    err = F.row_err(srdf, ref)
    print(f"MEASURE ray pairs RN={RN} SN={SN} {'rows' if pooled else 'slots'} precision={precision}: srdf worst ray {err:.2e} "
          f"(bound {SRDF_BOUND[precision]:.1e}); equal to tape build: {bool(torch.equal(srdf, tape))}; "
          f"equal to single-ray launches: {bool(torch.equal(srdf, alone))}")
    assert ops.status_poll(True) == 0                       # (d)
    assert bool(torch.isfinite(srdf).all())
    assert torch.equal(srdf, tape)                          # (a)
    assert err < SRDF_BOUND[precision]                      # (b)
    assert torch.equal(srdf, alone)                         # (c)


def _status_of(run):
    """the message of the sticky status a launch leaves behind (the bits are part of it), or None"""
    run()
    try:
        ops.status_poll(True)
    except UfrError as e:
        assert ops.status_poll(True) == 0                   # reporting clears it
        return str(e)
    return None


@pytest.mark.parametrize("precision", [FP32, LOWP], ids=["fp32", "16bit"])
@pytest.mark.parametrize("slot", [3, 20, 40], ids=["tile0", "tile1", "single_tile"])
def test_nan_token_raises_the_status_like_the_tape_build(slot, precision):
    """RN = 5, SN = 48 (pair + single): a NaN in one feature of one token of ray 4 (the partial workgroup), in the first or
    second tile of the pair or in the single tile of the last pass."""
    RN, SN, bad = 5, 48, 4
    token0, _ = _case(RN, SN)
    assert ops.status_poll(True) == 0
    clean = ops.ray_transform(_weights(), token0, RN, SN, precision=precision)
    tok = token0.clone()
    tok[bad * SN + slot, 11] = float("nan")
    out = {}
    fwd = _status_of(lambda: out.__setitem__("srdf", ops.ray_transform(_weights(), tok, RN, SN, precision=precision)))
    tape = _status_of(lambda: out.__setitem__("tape", _tape(tok, RN, SN, None, precision)))
    print(f"MEASURE NaN at slot {slot} precision={precision}: forward '{fwd}' / tape '{tape}'")
    assert fwd is not None and "NaN among" in fwd
    assert fwd == tape
    keep = [r for r in range(RN) if r != bad]
    assert torch.equal(out["srdf"][keep], clean[keep])      # rays are independent
    # the poisoned ray itself: NaN where the tape build has NaN, the same bits elsewhere (a ReLU drops a NaN)
    assert torch.equal(torch.nan_to_num(out["srdf"], nan=12345.0), torch.nan_to_num(out["tape"], nan=12345.0))
    assert ops.status_poll(True) == 0
