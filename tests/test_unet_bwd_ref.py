"""tests/unet_bwd_ref.py pinned, without a GPU: the restated geometry of csrc/conv3d_wgrad_planes.hip (every brick in exactly one
run at every workgroup count the launcher can choose, the job kinds tiling the gradient, the conditions WG_SHAPE and ONE_BRICK
must meet), the three evaluations of a layer's weight gradient against each other, and the comparison of
tests/test_gpu_conv3d_bwd_float64.py run on results that must pass (the model itself, float64 rounded to float32) and on
deliberately wrong ones of the kinds this kernel can produce (each must fail, and the message must name the kind or the tap)."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import unet_bwd_ref as R
from unet_bwd_ref import S1, S2, T2

ROW_IDS = [f"{ca}x{cb}-S{s}" for ca, cb, s in R.ROWS]


@functools.lru_cache(maxsize=None)
def _case(layer, shape=R.WG_SHAPE):
    x, d = R.layer_inputs(layer, shape, seed=1000 + 100 * layer[0] + layer[1] + layer[2])
    return x, d, R.references(x, d, layer[0])


# ----------------------------------------------------------------------------------------------------------------- geometry
def test_the_rows_are_the_layers_of_the_network():
    assert {R.row_of(l) for l in R.LAYERS} == set(R.ROWS) and len(R.ROWS) == 9
    assert R.HEADS_ROW in R.ROWS and R.kinds(R.HEADS_ROW) == 1          # the heads: nine rows of ONE 16-row tile, one kind
    assert sorted({R.kinds(r) for r in R.ROWS}) == [1, 3, 6, 12, 24]
    assert all(512 // R.kinds(r) >= 8 for r in R.ROWS)


@pytest.mark.parametrize("n_kinds", sorted({R.kinds(r) for r in R.ROWS}))
def test_run_partition_covers_every_brick_exactly_once(n_kinds):
    for n in range(1, 4001):
        blocks = R.blocks_per_kind(n, n_kinds)
        assert blocks % 8 == 0 and 8 <= blocks <= -(-(512 // n_kinds) // 8) * 8
        assert blocks < n / 4 + 8                                   # no more workgroups per kind than bricks / 4, but for the rounding
        runs = R.run_partition(n, blocks)
        assert len(runs) == blocks and all(b >= a for a, b in runs)
        chain = sorted(r for r in runs if r[1] > r[0])
        assert chain[0][0] == 0 and chain[-1][1] == n, n
        assert all(chain[i][1] == chain[i + 1][0] for i in range(len(chain) - 1)), n      # no gap, no brick twice
        for xcd in range(R.XCDS):                                   # a workgroup's XCD (w % 8) owns one contiguous eighth
            mine = [r for r in runs[xcd::R.XCDS] if r[1] > r[0]]
            assert all(mine[i][1] == mine[i + 1][0] for i in range(len(mine) - 1)), (n, xcd)


@pytest.mark.parametrize("row", list(R.ROWS), ids=ROW_IDS)
def test_kinds_tile_the_gradient_exactly_once(row):
    CA, CB, _ = row
    seen = torch.zeros(CA, CB, 27, dtype=torch.int32)
    for kind in range(R.kinds(row)):
        ra, rb, rt = R.kind_ranges(row, kind)
        assert len(ra) and len(rb) and len(rt)
        seen[ra.start:ra.stop, rb.start:rb.stop, rt.start:rt.stop] += 1
        assert all(R.kind_of(row, a, b, t) == R.kind_decode(row, kind) for a in (ra[0], ra[-1]) for b in (rb[0], rb[-1]) for t in (rt[0], rt[-1]))
    assert bool((seen == 1).all())
    # the taps whose tile ends in padding taps
    want = [26] if CB == 8 else list(range(16, 27)) if CB == 1 else []
    assert [t for t in range(27) if R.tap_shares_padding(row, t)] == want


@pytest.mark.parametrize("row", list(R.ROWS), ids=ROW_IDS)
def test_wg_shape_and_one_brick_meet_their_conditions(row):
    S = row[2]
    B, D, H, W = R.WG_SHAPE
    nbx, nby, nbz, per, total = R.bricks(row, R.WG_SHAPE)
    assert total == (54 if S == 1 else 81)
    blocks = R.blocks_per_kind(total, R.kinds(row))
    assert blocks == (16 if S == 1 else 24)
    runs = R.run_partition(total, blocks)
    assert {b - a for a, b in runs} == {3, 4}
    assert any(a // per != (b - 1) // per for a, b in runs)            # a run crosses from one batch element into the next
    # both remainders of the split are non-zero in some XCD
    q, r = divmod(total, 8)
    assert r != 0 and any((q + (1 if xcd < r else 0)) % (blocks // 8) for xcd in range(8))
    # bricks cut in x and y, and in z where a brick is two planes deep
    assert W % R.TX and H % R.TY and (D % 2 if S == 1 else R.cfg(row).TZ == 1)
    # a brick at place 2 of a run of 3 exists (the mutants below take it)
    assert any(b - a == 3 for a, b in runs)
    # ONE_BRICK: one brick, seven idle workgroups per kind
    assert R.bricks(row, R.ONE_BRICK)[4] == 1
    one = R.run_partition(1, R.blocks_per_kind(1, R.kinds(row)))
    assert len(one) == 8 and sorted(b - a for a, b in one) == [0] * 7 + [1]
    # the bricks' boxes tile the TP grid
    seen = torch.zeros(R.WG_SHAPE, dtype=torch.int32)
    for k in range(total):
        seen[R.brick_box(row, R.WG_SHAPE, k)] += 1
    assert bool((seen == 1).all())


def test_layer_shapes():
    assert R.in_shape((S2, 8, 16), R.WG_SHAPE) == (3, 6, 20, 140) and R.out_shape((S2, 8, 16), R.WG_SHAPE) == R.WG_SHAPE
    assert R.in_shape((T2, 16, 8), R.WG_SHAPE) == R.WG_SHAPE and R.out_shape((T2, 16, 8), R.WG_SHAPE) == (3, 6, 20, 140)
    assert R.in_shape((S1, 8, 8), R.WG_SHAPE) == R.out_shape((S1, 8, 8), R.WG_SHAPE) == R.WG_SHAPE


# -------------------------------------------------------------------------------------------------------- the three evaluators
@pytest.mark.parametrize("layer", [(S1, 8, 8), (S2, 8, 16), (T2, 16, 8)], ids=R.layer_id)
def test_wgrad_is_autograd_of_the_plain_convolution(layer):
    mode, cin, cout = layer
    x, d = R.layer_inputs(layer, (2, 2, 5, 9), seed=3)
    xn = x.double().permute(0, 4, 1, 2, 3)
    w = torch.randn(R.weight_shape(layer), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose3d(xn, w, b, stride=2, padding=1, output_padding=1) if mode == T2 else F.conv3d(xn, w, b, stride=2 if mode == S2 else 1, padding=1)
    y.backward(d.double().permute(0, 4, 1, 2, 3))
    dw, db = R.wgrad64(x, d, mode)
    assert torch.allclose(dw, w.grad, rtol=1e-12, atol=1e-12) and torch.allclose(db, b.grad, rtol=1e-12, atol=1e-12)
    # ... and it is the kernel's formulation: dW[a][b][k] = sum_p TP[p][a] TQ[S p + k - 1][b], checked at one tap of one pair
    S = 1 if mode == S1 else 2
    tp, tq = (x, d) if mode == T2 else (d, x)
    kz, ky, kx = 2, 0, 1
    acc = 0.0
    Bq, Dq, Hq, Wq, _ = tq.shape
    for bi in range(tp.shape[0]):
        for z in range(tp.shape[1]):
            for yy in range(tp.shape[2]):
                for xx in range(tp.shape[3]):
                    qz, qy, qx = S * z + kz - 1, S * yy + ky - 1, S * xx + kx - 1
                    if 0 <= qz < Dq and 0 <= qy < Hq and 0 <= qx < Wq:
                        acc += float(tp[bi, z, yy, xx, 1].double() * tq[bi, qz, qy, qx, 2].double())
    assert abs(float(dw[1, 2, kz, ky, kx]) - acc) < 1e-10 * max(1.0, abs(acc))


def test_split_is_two_bf16_planes_with_sixteen_bits():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(5)) * torch.tensor([2.0 ** -40, 1.0, 2.0 ** 30, 3.7]).repeat(1024)
    hi, lo = R.split_bf16(v)
    for t in (hi, lo):                      # bf16 numbers: the low 16 bits of the float32 are zero
        assert int((t.view(torch.int32) & 0xffff).abs().max()) == 0
    assert float(((hi.double() + lo.double() - v.double()).abs() / v.double().abs()).max()) <= 2.0 ** -17


@pytest.mark.parametrize("layer", R.LAYERS, ids=R.layer_id)
def test_model_is_within_the_row_bound_of_float64_and_the_comparison_accepts_it(layer):
    """The kernel's designed operand rounding, per row: at most 7e-6 measured, bound 2e-5.  `check_wgrad` accepts the model
    itself (as float32: what a kernel can return) and float64 rounded to float32."""
    x, d, ref = _case(layer)
    row = R.row_of(layer)
    e, _ = R.row_errors(ref.wm, ref.w64, ref.w64)
    y, _ = R.row_errors(ref.w32, ref.w64, ref.w64)
    eb = R.bias_errors(ref.bm, ref.b64, ref.b64, ref.mag)
    print(f"MEASURE {R.layer_id(layer)} at {R.WG_SHAPE}: model - float64 d weight {float(e.max()):.2e} (worst row)  d bias {float(eb.max()):.2e}  "
          f"float32 torch - float64 {float(y.max()):.2e}")
    assert float(e.max()) < R.ROW_BOUND and float(eb.max()) < R.ROW_BOUND
    assert float(e.max()) > 1e-6                    # ... and it is no small thing: a bound on the distance to float64 hides what is inside it
    R.check_wgrad("model", ref.wm.float(), ref.bm.float(), ref, row, bias_kernel="rides" if layer[0] != T2 else "channel sum")
    R.check_wgrad("float64 rounded", ref.w64.float(), ref.b64.float(), ref, row)


def test_power_of_two_scaling_is_exact_in_all_three_evaluations():
    """`scaled`: d_out times powers of two (a number, or one per channel) scales the float64, float32 and model gradients
    bit for bit -- the GPU tests evaluate the references once per layer and scale them."""
    for layer in [(S1, 8, 8), (T2, 16, 8)]:
        x, d = R.layer_inputs(layer, R.ONE_BRICK, seed=6)
        ref = R.references(x, d, layer[0])
        for s in (2.0 ** -40, 2.0 ** 30, R.channel_spread(layer[2])):
            want = R.references(x, (d.double() * torch.as_tensor(s, dtype=torch.float64)).float(), layer[0])
            got = R.scaled(ref, s, layer[0] != T2)
            for k in ("w64", "b64", "w32", "b32", "wm", "bm", "mag"):
                assert torch.equal(getattr(got, k), getattr(want, k)), (layer, k)


# ------------------------------------------------------------------------------------------------------------------ mutants
def _rejects(ref, row, w, b, pattern, rules=("i", "ii")):
    with pytest.raises(AssertionError) as ei:
        R.check_wgrad("mutant", w.float(), None if b is None else b.float(), ref, row, rules=rules)
    assert re.search(pattern, str(ei.value)), str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("layer", R.LAYERS, ids=R.layer_id)
def test_a_dropped_plane_product_is_rejected(layer):
    """contract3 without its a.p[1] b.p[0] product: 1e-3 .. 3e-3 of a row -- far below what the analytic worst case of the
    operand rounding allows at 1e5 voxels per weight"""
    x, d, ref = _case(layer)
    w, b = R.wgrad_model(x, d, layer[0], drop="tp_lo.tq_hi")
    e, _ = R.row_errors(w, ref.wm, ref.w64)
    print(f"MEASURE {R.layer_id(layer)}: lo.hi dropped moves the worst row by {float(e.max()):.2e}, the best by {float(e.min()):.2e}")
    assert 5e-4 < float(e.min()) and float(e.max()) < 5e-3
    _rejects(ref, R.row_of(layer), w, b, r"\(i\) \d+ of \d+ rows")


def _brick_at_place_2_of_3(row):
    total = R.bricks(row, R.WG_SHAPE)[4]
    runs = R.run_partition(total, R.blocks_per_kind(total, R.kinds(row)))
    return next(a + 2 for a, b in runs if b - a == 3)


@pytest.mark.parametrize("layer", [(S1, 8, 8), (S1, 1, 8), (S1, 64, 64), (S2, 16, 32), (T2, 16, 8)], ids=R.layer_id)
@pytest.mark.parametrize("times", [0, 2], ids=["missing", "twice"])
def test_a_brick_late_in_a_run_missing_or_counted_twice_is_rejected(layer, times):
    x, d, ref = _case(layer)
    row = R.row_of(layer)
    k = _brick_at_place_2_of_3(row)
    cw, cb = R.wgrad_model(*R.tp_masked_to_brick(layer, R.WG_SHAPE, x, d, k), layer[0])
    if layer[0] == T2:
        cb = torch.zeros_like(cb)           # channel_sum_kernel's bias knows no bricks
    _rejects(ref, row, ref.wm + (times - 1) * cw, ref.bm + (times - 1) * cb, r"\(i\) \d+ of \d+ rows")
    # the brick's part and the rest are the whole: the masking is the brick's contribution
    rest = torch.zeros_like(ref.wm)
    if layer == (S1, 8, 8):
        for kk in range(R.bricks(row, R.WG_SHAPE)[4]):
            rest += R.wgrad64(*R.tp_masked_to_brick(layer, R.WG_SHAPE, x, d, kk), layer[0])[0]
        assert torch.allclose(rest, ref.w64, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("layer,kind", [((S1, 32, 32), 4), ((S1, 64, 64), 17), ((S2, 16, 32), 2), ((T2, 64, 32), 7)],
                         ids=lambda v: R.layer_id(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("factor", [0.0, 2.0], ids=["zero", "doubled"])
def test_one_job_kinds_block_zero_or_doubled_is_rejected_and_named(layer, kind, factor):
    """a kind that never flushed / a block flushed by two kinds"""
    x, d, ref = _case(layer)
    row = R.row_of(layer)
    ra, rb, rt = R.kind_ranges(row, kind)
    w = ref.wm.clone().flatten(2)
    w[ra.start:ra.stop, rb.start:rb.stop, rt.start:rt.stop] *= factor
    ag, bb, tg = R.kind_decode(row, kind)
    msg = _rejects(ref, row, w.view_as(ref.wm), ref.bm, rf"job kind {kind} \(ag {ag}, bb {bb}, tg {tg}\)")
    assert f"{len(ra)} of {row[0]} rows" in msg        # exactly the kind's rows


@pytest.mark.parametrize("layer", [(S1, 8, 8), (S1, 8, 1), (S2, 8, 16), (T2, 16, 8)], ids=R.layer_id)
def test_the_padding_tap_added_into_tap_26_is_rejected_and_named(layer):
    """CB = 8: the second half of the fourteenth pair is padding tap 27, which reads the voxel of tap 0; flushed without the
    `tap < 27` guard into its neighbour it lands on tap 26"""
    x, d, ref = _case(layer)
    row = R.row_of(layer)
    assert row[1] == 8
    w = ref.wm.clone().flatten(2)
    w[:, :, 26] += w[:, :, 0]
    _rejects(ref, row, w.view_as(ref.wm), ref.bm, r"\[tap=26\].*tap 26 is the last of a pair, beside padding tap 27")


def test_a_padding_tap_of_the_one_channel_tile_is_named():
    """CB = 1: taps 16 .. 26 share their tile with padding taps 27 .. 31"""
    layer = (S1, 1, 8)
    x, d, ref = _case(layer)
    w = ref.wm.clone().flatten(2)
    w[:, :, 20] += w[:, :, 0]
    _rejects(ref, R.row_of(layer), w.view_as(ref.wm), ref.bm, r"\[tap=20\].*in the tile that ends in padding taps 27 \.\. 31")


@pytest.mark.parametrize("layer", [(S1, 8, 8), (S1, 64, 64), (S2, 8, 16), (T2, 16, 8)], ids=R.layer_id)
def test_a_doubled_bias_is_rejected(layer):
    x, d, ref = _case(layer)
    msg = _rejects(ref, R.row_of(layer), ref.wm, 2 * ref.bm, r"\(i\) d bias\[\d+\]")
    assert "dW[" not in msg


def test_an_error_confined_to_the_smallest_row_needs_the_per_row_metric():
    """d_out channel c at 2^(-5 c): 1e-3 of the smallest row is 3e-14 of the tensor's maximum.  The old whole-tensor metric
    passes it at any bound it ever held; the per-row rules reject it, (i) and (ii) both."""
    layer = (S1, 8, 8)
    x, d, unit = _case(layer)
    ref = R.scaled(unit, R.channel_spread(8), True)
    row = R.row_of(layer)
    R.check_wgrad("spread model", ref.wm.float(), ref.bm.float(), ref, row)
    w = ref.wm.clone()
    w[7] *= 1.0 + 1e-3
    assert R.tensor_error(w.float(), ref.w64) < 2e-5                    # the old metric and the old bound: not seen
    assert abs(R.tensor_error(w.float(), ref.w64) - R.tensor_error(ref.wm.float(), ref.w64)) < 1e-12
    msg = _rejects(ref, row, w, ref.bm, r"\(i\) 1 of 8 rows.*dW\[a=7\]")
    assert "(ii) 1 of 8 rows" in msg
    # the same for one bias element
    b = ref.bm.clone()
    b[7] *= 1.0 + 1e-3
    assert R.tensor_error(b.float(), ref.b64) < 2e-5
    _rejects(ref, row, ref.wm, b, r"\(i\) d bias\[7\]")


# ------------------------------------------------------------------------------------------------------------ the whole network
def test_net_gradients_run_on_a_copy_and_follow_the_frozen_set():
    class Net(torch.nn.Module):         # CostRegNetWeight's layers (uforecon_amd.cascade), here so that nothing of the package is imported
        def __init__(self):
            super().__init__()
            ch = [8, 16, 32, 64]
            self.conv0 = torch.nn.Conv3d(1, 8, 3, padding=1)
            for lvl in (1, 2, 3):
                setattr(self, f"conv{2 * lvl - 1}", torch.nn.Conv3d(ch[lvl - 1], ch[lvl], 3, stride=2, padding=1))
                setattr(self, f"conv{2 * lvl}", torch.nn.Conv3d(ch[lvl], ch[lvl], 3, padding=1))
            for name, lvl in (("conv7", 3), ("conv9", 2), ("conv11", 1)):
                setattr(self, name, torch.nn.ConvTranspose3d(ch[lvl], ch[lvl - 1], 3, stride=2, padding=1, output_padding=1))
            self.features = torch.nn.Conv3d(8, 8, 3, padding=1, bias=False)
            self.weights = torch.nn.Conv3d(8, 1, 3, padding=1, bias=False)

    torch.manual_seed(7)
    m = Net()
    x = torch.randn(1, 1, 8, 8, 16)
    loss = lambda f, w: (f * f).mean() + w.sum()
    g64 = R.net_gradients(m, x, loss, torch.float64)
    g32 = R.net_gradients(m, x, loss, torch.float32)
    assert all(p.grad is None and p.dtype == torch.float32 for p in m.parameters())
    assert set(g64) == {k for k, _ in m.named_parameters()} | {"x"} and len(g64) == 23
    assert all(g64[k].dtype == torch.float64 and R.tensor_rel(g32[k], g64[k]) < 1e-4 for k in g64)
    fr = R.net_gradients(m, x, loss, torch.float64, frozen=("conv4.weight", "conv4.bias", "features.weight"), x_grad=False)
    assert fr["conv4.weight"] is None and fr["conv4.bias"] is None and fr["features.weight"] is None and fr["x"] is None
    assert all(torch.equal(fr[k], g64[k]) for k in g64 if fr[k] is not None)
    R.rows_close("same", g32["conv2.weight"], g64["conv2.weight"].float(), g64["conv2.weight"], g32["conv2.weight"])
    with pytest.raises(AssertionError, match="row 3 differs"):
        bad = g64["conv2.weight"].clone()
        bad[3] *= 1.001
        R.rows_close("one row off", bad, g64["conv2.weight"], g64["conv2.weight"], g32["conv2.weight"])


def test_an_error_confined_to_the_smallest_column_of_a_transposed_layer_needs_the_per_column_rules():
    """The transposed layer's d_out is TQ: its small channels are COLUMNS of dW, and every row's maximum sits in column 0.
    The per-row rules pass 1e-3 of the smallest column; with ``columns`` it is rejected and named."""
    layer = (T2, 16, 8)
    x, d, unit = _case(layer)
    ref = R.scaled(unit, R.channel_spread(8), False)
    row = R.row_of(layer)
    R.check_wgrad("spread model", ref.wm.float(), ref.bm.float(), ref, row, bias_kernel="channel sum", columns=True)
    w = ref.wm.clone()
    w[:, 7] *= 1.0 + 1e-3
    R.check_wgrad("rows alone", w.float(), ref.bm.float(), ref, row, bias_kernel="channel sum")
    with pytest.raises(AssertionError, match=r"\(i\) 1 of 8 columns.*dW\[a=\d+\]\[b=7\].*of column 7's scale"):
        R.check_wgrad("columns too", w.float(), ref.bm.float(), ref, row, bias_kernel="channel sum", columns=True)
