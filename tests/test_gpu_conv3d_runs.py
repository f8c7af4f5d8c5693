"""The U-Net plane kernels (csrc/conv3d_planes.hip) where a persistent workgroup walks a RUN of bricks -- the state every
full-resolution layer of a real frame is in, and which no other test reaches (their launches have fewer bricks than resident
workgroups: one brick each) -- and the fp32 kernels that stay on the product path (csrc/conv3d.hip), against float64.

Shapes: tests/unet_ref.py RUN_SHAPES, one per instantiation: 2 .. 3 bricks per workgroup, both remainders of the XCD-aware split,
runs that cross batch elements, bricks cut at the edge (tests/test_unet_ref.py asserts it, and that the comparison rejects a wrong
brick late in a run).  THE RULE of every float64 assertion: err(kernel) < max(4 err(torch float32 on the CPU), 1e-6) of the output
scale -- the yardstick is torch's, none of the project's kernels.  Every call under test is preceded by a NaN-filled allocation of
its output's size (the caching allocator then hands NaN, not an earlier call's correct values, to the kernel's torch.empty) and
runs before anything else computes the same output.  Every pair is printed as a MEASURE line.
"""
import copy
import functools

import pytest
import torch

import unet_ref as R
from unet_ref import S1, S2, T2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

VARIANTS = [(inst, v) for inst in R.INSTANTIATIONS for v in ("plain", "bias+skip", "bn+relu+skip") if v != "bn+relu+skip" or inst[0] != T2]
S1_INSTS = [i for i in R.INSTANTIATIONS if i[0] == S1]


@functools.lru_cache(maxsize=2)
def _inputs(inst):
    return R.layer_inputs(inst, R.RUN_SHAPES[inst], seed=100 * inst[0] + inst[1], device=DEV)


def _planes(x, amax, w, mode=S1, **kw):
    """ufr_conv3d_planes into a poisoned block"""
    from uforecon_amd import ops

    B, D, H, W, _ = x.shape
    cout = w.shape[1] if (mode == T2 or kw.get("flip")) else w.shape[0]
    out = (B, *R.out_extent(mode, (D, H, W)))
    R.poison(DEV, (*out, cout), *([] if kw.get("weight2") is None else [(*out, kw["weight2"].shape[0])]))
    return ops.conv3d_planes(x, amax, w, mode=mode, **kw)


def _per_element(x, amax, w, mode=S1, skip=None, **kw):
    """The same layer as B launches of one batch element each (one brick per workgroup: the state the rest of the suite
    pins), every one with the whole tensor's bound and the same weight tensor."""
    outs = [_planes(x[b:b + 1], amax, w, mode, skip=None if skip is None else skip[b:b + 1], **kw) for b in range(x.shape[0])]
    return [torch.cat([o[i] for o in outs]) if outs[0][i] is not None else None for i in range(len(outs[0]))]


def _assert_same_bits(label, got, want, inst, shape, ncdhw=False):
    if not torch.equal(got, want):
        be = R.brick_errors(got, want, inst[0], inst[1], shape, ncdhw)
        raise AssertionError(f"{label}: one launch over the runs differs from the single-element launches -- "
                             + R.describe_bricks(be, inst[0], inst[1], shape, 1e-30))


@pytest.mark.parametrize("shapes", [[(2, 3, 10, 66, 8)], [(7, 22, 118, 34, 16)], [(2, 8, 3, 10, 66), (2, 1, 3, 10, 66)]], ids=["small", "large", "pair"])
def test_poison_reaches_the_next_allocations(shapes):
    """The guard itself: what `torch.empty` hands out after `poison` is NaN throughout, in the kernels' allocation order."""
    stale = [torch.ones(s, device=DEV) for s in shapes]          # freed blocks of the same sizes, holding finite values
    del stale
    R.poison(DEV, *shapes)
    got = [torch.empty(s, dtype=torch.float32, device=DEV) for s in shapes]
    assert all(bool(torch.isnan(t).all()) for t in got)


# ------------------------------------------------------------------------------------------------ a. runs against float64
@pytest.mark.parametrize("inst,variant", VARIANTS, ids=[f"{R.inst_id(i)}-{v}" for i, v in VARIANTS])
def test_runs_match_float64(inst, variant):
    from uforecon_amd import ops

    mode, cin = inst
    shape = R.RUN_SHAPES[inst]
    x, w, bias, sc, sh, skip = _inputs(inst)
    kw = {"plain": {}, "bias+skip": dict(bias=bias, skip=skip), "bn+relu+skip": dict(bn_scale=sc, bn_shift=sh, relu=True, skip=skip)}[variant]
    y, ymax = _planes(x, ops.absmax(x), w, mode, **kw)
    assert float(ymax) == float(y.abs().max())                  # the bound handed to the next layer is the true maximum
    R.check(f"runs {R.inst_id(inst)} {variant} {shape}", y, R.layer64(x, w, mode, **kw), R.layer32(x, w, mode, **kw), inst, shape)


# ----------------------------------------------------------------------------- b. runs equal single bricks, bit for bit
@pytest.mark.parametrize("inst", R.INSTANTIATIONS, ids=R.inst_id)
def test_runs_equal_single_element_launches_bit_for_bit(inst):
    from uforecon_amd import ops

    mode, cin = inst
    shape = R.RUN_SHAPES[inst]
    x, w, bias, sc, sh, skip = _inputs(inst)
    amax = ops.absmax(x)
    y, ymax = _planes(x, amax, w, mode, bias=bias, skip=skip)
    y1, m1 = _per_element(x, amax, w, mode, bias=bias, skip=skip)
    assert not bool(torch.isnan(y1).any())
    _assert_same_bits(R.inst_id(inst), y, y1, inst, shape)
    assert float(ymax) == float(m1.max()) == float(y1.abs().max())


# ------------------------------------------------------------------------------------- c. the remaining forms at a run shape
@pytest.mark.parametrize("inst", S1_INSTS, ids=R.inst_id)
def test_runs_of_the_mirrored_form_match_float64(inst):
    """flip: the data gradient of a stride-1 layer (mirrored taps on the forward weight), a second gradient path accumulated"""
    from uforecon_amd import ops

    shape = R.RUN_SHAPES[inst]
    x, w, bias, sc, sh, skip = _inputs(inst)
    wf = w.clone()                                       # (cin, cout, 3,3,3) with cin = cout: read as the layer's FORWARD weight
    y, ymax = _planes(x, ops.absmax(x), wf, S1, flip=True, skip=skip)
    assert float(ymax) == float(y.abs().max())
    R.check(f"runs {R.inst_id(inst)} flip {shape}", y, R.layer64(x, wf, S1, flip=True, skip=skip), R.layer32(x, wf, S1, flip=True, skip=skip),
            inst, shape)


def test_runs_of_the_two_heads_match_float64_and_single_element_launches():
    """features (8) + sigmoid(weights (1)) in one pass, (B,C,D,H,W) outputs"""
    from uforecon_amd import ops

    inst = (S1, 8)
    shape = R.RUN_SHAPES[inst]
    x, w, *_ = _inputs(inst)
    g = torch.Generator().manual_seed(21)
    ww = (torch.randn(1, 8, 3, 3, 3, generator=g) * 0.1).to(DEV)
    amax = ops.absmax(x)
    f, s, _ = _planes(x, amax, w, S1, out_ncdhw=True, weight2=ww)
    assert f.shape == (shape[0], 8, *shape[1:]) and s.shape == (shape[0], 1, *shape[1:])
    f1, s1, _ = _per_element(x, amax, w, S1, out_ncdhw=True, weight2=ww)
    _assert_same_bits("heads, features", f, f1, inst, shape, ncdhw=True)
    _assert_same_bits("heads, weights", s, s1, inst, shape, ncdhw=True)
    rf, rs = R.layer64(x, w, S1, out_ncdhw=True, weight2=ww)
    yf, ys = R.layer32(x, w, S1, out_ncdhw=True, weight2=ww)
    R.check(f"runs heads features {shape}", f, rf, yf, inst, shape, ncdhw=True)
    R.check(f"runs heads sigmoid(weights) {shape}", s, rs, ys, inst, shape, ncdhw=True)


def test_runs_of_the_prob_layer_match_float64_and_single_element_launches():
    """cost_reg_net's last layer: 8 -> 1, (B,1,D,H,W)"""
    from uforecon_amd import ops

    inst = (S1, 8)
    shape = R.RUN_SHAPES[inst]
    x = _inputs(inst)[0]
    g = torch.Generator().manual_seed(22)
    wp = (torch.randn(1, 8, 3, 3, 3, generator=g) * 0.1).to(DEV)
    amax = ops.absmax(x)
    p, none = _planes(x, amax, wp, S1, out_ncdhw=True)
    assert none is None and p.shape == (shape[0], 1, *shape[1:])
    p1 = _per_element(x, amax, wp, S1, out_ncdhw=True)[0]
    _assert_same_bits("prob", p, p1, inst, shape, ncdhw=True)
    R.check(f"runs prob {shape}", p, R.layer64(x, wp, S1, out_ncdhw=True), R.layer32(x, wp, S1, out_ncdhw=True), inst, shape, ncdhw=True)


# ------------------------------------------------------------------------------------------------------------ d. an outlier
@pytest.mark.parametrize("inst", [(S1, 8), (S1, 16)], ids=R.inst_id)
def test_one_outlier_voxel_leaves_the_rest_of_the_volume_within_the_rule(inst):
    """One input voxel x 2^12: the planes' scale follows it (the tensor's measured maximum), every other voxel's planes lose
    12 bits of fp16 exponent range -- and none of their 22 significand bits.  The rule on the outputs outside the outlier's
    3 x 3 x 3 neighbourhood, of THEIR scale."""
    from uforecon_amd import ops

    shape = R.RUN_SHAPES[inst]
    x, w, bias, sc, sh, skip = _inputs(inst)
    x = x.clone()
    b0, z0, y0, x0 = 3, 5, 30, shape[3] // 2
    x[b0, z0, y0, x0] *= 4096.0
    keep = torch.ones((*shape, R.COUT[inst]), dtype=torch.bool, device=DEV)
    keep[b0, z0 - 1:z0 + 2, y0 - 1:y0 + 2, x0 - 1:x0 + 2] = False
    amax = ops.absmax(x)
    assert float(amax) == float(x.abs().max()) > 1000.0
    y, ymax = _planes(x, amax, w, S1, bias=bias, skip=skip)
    assert float(ymax) == float(y.abs().max())
    R.check(f"outlier 2^12 {R.inst_id(inst)} {shape}, outside its neighbourhood", y, R.layer64(x, w, S1, bias=bias, skip=skip),
            R.layer32(x, w, S1, bias=bias, skip=skip), inst, shape, keep=keep)


# --------------------------------------------------------------------------- e. the fp32 kernels that stay on the product path
E_SHAPE = (2, 3, 5, 523)       # odd extents; a grid row (523 voxels) is more than one 256-thread block at two voxels per thread


def _e_inputs(cin, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*E_SHAPE, cin, generator=g) * 2.0).to(DEV), g


@pytest.mark.parametrize("variant", ["bias", "bn+relu"])
def test_conv0_on_the_fp32_kernel_matches_float64_and_returns_the_exact_bound(variant):
    """conv0 (1 -> 8) with want_absmax: the bound conv1's planes scale by, on every U-Net call -- and, asked for, the reason the
    vector kernel runs.  Into a fresh zero word and into a pool slot that is not the first of its buffer (unet3d._Bounds)."""
    from uforecon_amd import ops

    x, g = _e_inputs(1, 31)
    w = (torch.randn(8, 1, 3, 3, 3, generator=g) * 0.3).to(DEV)
    bias, sc, sh = (t.to(DEV) for t in (torch.randn(8, generator=g), torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)))
    kw = dict(bias=bias) if variant == "bias" else dict(bn_scale=sc, bn_shift=sh, relu=True)
    R.poison(DEV, (*E_SHAPE, 8))
    y, ymax = ops.conv3d(x, w, ops.CONV3D_S1, want_absmax=True, **kw)
    assert ymax.shape == (1,) and float(ymax) == float(y.abs().max())
    R.check(f"fp32 kernel conv0 {variant} {E_SHAPE}", y, R.layer64(x, w, S1, **kw), R.layer32(x, w, S1, **kw))
    pool = torch.zeros(64, dtype=torch.float32, device=DEV)
    R.poison(DEV, (*E_SHAPE, 8))
    y2, slot = ops.conv3d(x, w, ops.CONV3D_S1, want_absmax=pool[5:6], **kw)
    assert torch.equal(y2, y) and float(pool[5]) == float(slot) == float(y.abs().max())
    assert int((pool != 0).sum()) == 1                     # and no other slot was touched


def test_prob_head_on_the_fp32_kernel_matches_float64():
    from uforecon_amd import ops

    x, g = _e_inputs(8, 32)
    w = (torch.randn(1, 8, 3, 3, 3, generator=g) * 0.1).to(DEV)
    R.poison(DEV, (E_SHAPE[0], 1, *E_SHAPE[1:]))
    y = ops.conv3d(x, w, ops.CONV3D_S1, out_ncdhw=True)
    assert y.shape == (E_SHAPE[0], 1, *E_SHAPE[1:])
    R.check(f"fp32 kernel 8 -> 1 (B,1,D,H,W) {E_SHAPE}", y, R.layer64(x, w, S1, out_ncdhw=True), R.layer32(x, w, S1, out_ncdhw=True))


def test_data_gradients_on_the_fp32_kernel_match_float64():
    """The two data gradients CostRegNetWeightFn.backward takes from csrc/conv3d.hip: the 1-channel head's (8 <- 1, with a second
    gradient accumulated) and conv0's (1 <- 8)."""
    from uforecon_amd import ops

    d1, g = _e_inputs(1, 33)
    w_head = (torch.randn(1, 8, 3, 3, 3, generator=g) * 0.1).to(DEV)
    acc = torch.randn(*E_SHAPE, 8, generator=g).to(DEV)
    R.poison(DEV, (*E_SHAPE, 8))
    got = ops.conv3d_bwd_data(d1, w_head, ops.CONV3D_S1, (*E_SHAPE, 8), accumulate=acc)
    R.check(f"fp32 kernel d in of the weights head (8 <- 1, accumulate) {E_SHAPE}", got, R.layer64(d1, w_head, S1, flip=True, skip=acc),
            R.layer32(d1, w_head, S1, flip=True, skip=acc))
    d8, g = _e_inputs(8, 34)
    w0 = (torch.randn(8, 1, 3, 3, 3, generator=g) * 0.1).to(DEV)
    R.poison(DEV, (*E_SHAPE, 1))
    got = ops.conv3d_bwd_data(d8, w0, ops.CONV3D_S1, (*E_SHAPE, 1))
    assert got.shape == (*E_SHAPE, 1)
    R.check(f"fp32 kernel d in of conv0 (1 <- 8) {E_SHAPE}", got, R.layer64(d8, w0, S1, flip=True), R.layer32(d8, w0, S1, flip=True))


# ----------------------------------------------------------------------------------- f. both networks, forward, against float64
NET_SHAPE = (3, 1, 8, 128, 192)         # levels 0 and 1 walk runs: 1152 and 576 bricks
NET_BOUND = 1e-5                        # the project's bound on a whole U-Net (tests/test_gpu_conv3d_bwd.py), here against float64;
                                        # beside it THE RULE with the float32 torch module on the CPU as the yardstick


def _net_check(label, outs, refs, yards):
    for name, o, r, y in zip(("features / cost", "sigmoid(weights)"), outs, refs, yards):
        e, e32 = R.err(o, r), R.err(y, r)
        print(f"MEASURE {label} {name} {NET_SHAPE}: kernels {e:.2e}  float32 torch module {e32:.2e}  ratio {e / e32:.2f}  "
              f"rule {'holds' if e < R.bound(e32) else 'does NOT hold'}")
        assert e < NET_BOUND, (label, name, e)
        assert e < R.bound(e32), (label, name, e, e32)      # measured on the MI355X: 0.6 .. 0.75 of torch's own distance -- the rule holds


@pytest.mark.parametrize("net", ["CostRegNet", "CostRegNetWeight"])
def test_whole_unet_forward_matches_float64(net):
    from oracle import cascade_oracle as CO
    from uforecon_amd import cascade
    from uforecon_amd.scene import fill_state_dict

    m = getattr(cascade, net)(1, 8)
    fill_state_dict(m, 17)              # BatchNorm weights, biases AND running statistics away from the identity
    m.eval()
    if net == "CostRegNet":
        assert float((m.conv1.bn.running_mean).abs().max()) > 0 and float((m.conv1.bn.running_var - 1).abs().max()) > 0
    m32, m64 = copy.deepcopy(m), copy.deepcopy(m).double().to(DEV)
    m = m.to(DEV)
    oracle = CO.cost_reg_net if net == "CostRegNet" else CO.cost_reg_net_weight
    x = torch.randn(NET_SHAPE, generator=torch.Generator().manual_seed(18)).to(DEV)
    tup = lambda t: t if isinstance(t, tuple) else (t,)
    with torch.no_grad():
        R.poison(DEV, (NET_SHAPE[0], 8, *NET_SHAPE[2:]), NET_SHAPE)
        outs = tup(m(x))
        refs = tup(oracle(m64, x.double()))
        yards = tup(oracle(m32, x.cpu()))
        _net_check(net, outs, refs, yards)
        again = tup(m(x))
    assert all(torch.equal(a, b) for a, b in zip(outs, again))


# --------------------------------------------------------------------- g. weight gradients at matrix-core sizes against float64
@pytest.mark.parametrize("mode,cin,cout,dims", [(S1, 16, 16, (16, 64, 104)), (S2, 16, 32, (32, 128, 208)), (T2, 32, 16, (16, 64, 104))])
def test_weight_gradients_at_matrix_core_sizes_match_float64(mode, cin, cout, dims):
    """The smallest case of each mode of test_gpu_conv3d_bwd.py::test_weight_gradients_at_matrix_core_sizes (same inputs), against
    float64 autograd at the 2e-5 that test_weight_gradient_on_the_matrix_cores_matches_float64 holds at small shapes: the 1e-4
    there bounds torch's fp32 sum of 1e5 terms as much as the kernel's."""
    from uforecon_amd import ops

    g = torch.Generator().manual_seed(cin * 100 + cout + mode)
    D, H, W = dims
    x = torch.randn(1, cin, D, H, W, generator=g).to(DEV)
    if mode == T2:
        conv = torch.nn.ConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1)
    else:
        conv = torch.nn.Conv3d(cin, cout, 3, stride=2 if mode == S2 else 1, padding=1)
    conv = conv.double().to(DEV)
    y = conv(x.double())
    d_out = torch.randn(y.shape, generator=g).to(DEV)
    y.backward(d_out.double())
    cl = lambda t: t.detach().permute(0, 2, 3, 4, 1).contiguous()
    dw, db = ops.conv3d_bwd_weight(cl(x), cl(d_out), mode, conv.weight.shape)
    ew, eb = R.err(dw, conv.weight.grad), R.err(db, conv.bias.grad)
    print(f"MEASURE wgrad {R.MODE_NAMES[mode]} {cin} -> {cout} {dims}: d weight {ew:.2e}  d bias {eb:.2e} of scale, against float64 autograd")
    assert ew < 2e-5 and eb < 2e-5
