"""The backward of the trainable frustum U-Net against float64: the weight-gradient plane kernels
(csrc/conv3d_wgrad_planes.hip: all nine instantiations in both roles of the stride-2 rows, and the two-heads form) and
`unet3d.CostRegNetWeightFn`.  Every reference is computed on the CPU (tests/unet_bwd_ref.py): nothing on the right-hand side of
an assertion ran on the GPU.

Shapes: WG_SHAPE -- 54 / 81 bricks on 16 / 24 workgroups per job kind, runs of 3 and 4 bricks that cross batch elements, both
remainders of the split, bricks cut in x, y (and z) -- and ONE_BRICK, where seven workgroups per kind have nothing to flush
(tests/test_unet_bwd_ref.py asserts these conditions, and that the comparison rejects a dropped plane product, a brick missing or
twice, a kind's block zero or doubled, a padding tap flushed, a doubled bias).  `check_wgrad` holds, PER ROW of dW[a][b][tap]
(and per column for the transposed layers, whose d_out channels are columns): (i) |kernel - model of its operand arithmetic| <
max(4 |torch float32 - float64|, 1e-6) and (ii) |kernel - float64| < 2e-5.
Every figure is printed as a MEASURE line.
"""
import copy
import functools

import pytest
import torch

import unet_bwd_ref as R
from unet_bwd_ref import S1, S2, T2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"runs": R.WG_SHAPE, "one-brick": R.ONE_BRICK}


@functools.lru_cache(maxsize=None)
def _case(layer, shape="runs", positive_input=False):
    """(x_cl, d_cl) on the CPU and their references, evaluated once per layer and shape"""
    x, d = R.layer_inputs(layer, SHAPES[shape], seed=2000 + 100 * layer[0] + layer[1] + layer[2] + (7 if positive_input else 0),
                          positive_input=positive_input)
    return x, d, R.references(x, d, layer[0])


def _launch(layer, x, d, **kw):
    from uforecon_amd import ops

    return ops.conv3d_bwd_weight(x.to(DEV), d.to(DEV), layer[0], R.weight_shape(layer), **kw)


def _bias_kernel(layer):
    return "channel sum" if layer[0] == T2 else "rides"


# ------------------------------------------------------------------------------------- a. every instantiation, runs and one brick
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("layer", R.LAYERS, ids=R.layer_id)
def test_weight_gradient_matches_its_model_and_float64(layer, shape):
    x, d, ref = _case(layer, shape)
    dw, db = _launch(layer, x, d)
    assert dw.shape == R.weight_shape(layer) and db.shape == (layer[2],)
    R.check_wgrad(f"wgrad {R.layer_id(layer)} {shape} {SHAPES[shape]}", dw, db, ref, R.row_of(layer), bias_kernel=_bias_kernel(layer), columns=layer[0] == T2)


# ------------------------------------------------------------------------------------------ b. the magnitudes training produces
def _magnitude(layer, variant):
    """-> (x, d, references) with d_out at the variant's magnitude.  Powers of two scale all three evaluations exactly
    (`R.scaled`), so the unit case's references serve; the factors stay far from bf16's and fp32's subnormal range."""
    if variant == "positive-input":
        return _case(layer, "runs", True)
    x, d, ref = _case(layer)
    s = {"2^-40": torch.tensor(2.0 ** -40, dtype=torch.float64), "2^30": torch.tensor(2.0 ** 30, dtype=torch.float64),
         "channel-spread": R.channel_spread(layer[2])}[variant]
    return x, (d.double() * s).float(), R.scaled(ref, s, layer[0] != T2)


@pytest.mark.parametrize("variant", ["2^-40", "2^30", "channel-spread", "positive-input"])
@pytest.mark.parametrize("layer", R.LAYERS, ids=R.layer_id)
def test_weight_gradient_at_training_magnitudes(layer, variant):
    """Unscaled small gradients, a loss scaler, d_out channel c at 2^(-5 c) (capped at 2^-40: every row against its own
    maximum, and for the transposed layers, whose d_out is TQ, every column), and a layer input with a positive mean (sums
    that do not cancel): the same relative bounds."""
    x, d, ref = _magnitude(layer, variant)
    dw, db = _launch(layer, x, d)
    R.check_wgrad(f"wgrad {R.layer_id(layer)} {variant}", dw, db, ref, R.row_of(layer), bias_kernel=_bias_kernel(layer), columns=layer[0] == T2)


# ------------------------------------------------------------------------------------------------------------ c. the two heads
def _heads_inputs(scale2):
    x, d, ref = _case((S1, 8, 8))
    d2 = torch.randn(*R.WG_SHAPE, 1, generator=torch.Generator().manual_seed(31)) * scale2
    return x, d, d2, ref, R.references(x, d2, S1)


def test_heads_with_a_saturated_sigmoid():
    """d_out2 at 2^-20 of d_out: the ninth row of the shared tile against its own model and its own maximum"""
    from uforecon_amd import ops

    x, d, d2, ref, ref2 = _heads_inputs(2.0 ** -20)
    gf, gw = ops.conv3d_bwd_weight_heads(x.to(DEV), d.to(DEV), d2.to(DEV))
    assert gf.shape == (8, 8, 3, 3, 3) and gw.shape == (1, 8, 3, 3, 3)
    R.check_wgrad("heads, features (d_out2 at 2^-20)", gf, None, ref, (8, 8, 1))
    R.check_wgrad("heads, weights (d_out2 at 2^-20)", gw, None, ref2, (1, 8, 1))


def test_heads_equal_the_two_single_launches():
    from uforecon_amd import ops

    x, d, d2, ref, ref2 = _heads_inputs(1.0)
    gf, gw = ops.conv3d_bwd_weight_heads(x.to(DEV), d.to(DEV), d2.to(DEV))
    sf = _launch((S1, 8, 8), x, d, want_bias=False)[0]
    sw = _launch((S1, 8, 1), x, d2, want_bias=False)[0]
    R.check_wgrad("heads, features", gf, None, ref, (8, 8, 1))
    R.check_wgrad("heads, weights", gw, None, ref2, (1, 8, 1))
    R.check_wgrad("heads, features against the single launch", gf, None, ref, (8, 8, 1), centre_w=sf.cpu(), rules=("i",))
    R.check_wgrad("heads, weights against the single launch", gw, None, ref2, (1, 8, 1), centre_w=sw.cpu(), rules=("i",))


# ----------------------------------------------------------------------------------------------------- d. "accumulated into"
@pytest.mark.parametrize("layer", [(S1, 1, 8), (S1, 8, 8), (S1, 64, 64), (S2, 16, 32), (T2, 16, 8)], ids=R.layer_id)
def test_results_are_accumulated_into(layer):
    """A second call into the same `out=` tensors gives twice the first; `want_bias=False` gives no bias and the same
    weight gradient (but for the order of the atomics): rule (i)."""
    x, d, ref = _case(layer)
    row = R.row_of(layer)
    dw, db = _launch(layer, x, d)
    first_w, first_b = dw.clone().cpu(), db.clone().cpu()
    dw2, db2 = _launch(layer, x, d, out=(dw, db))
    assert dw2.data_ptr() == dw.data_ptr() and db2.data_ptr() == db.data_ptr()
    R.check_wgrad(f"wgrad {R.layer_id(layer)} second call / 2", dw / 2, db / 2, ref, row, centre_w=first_w, centre_b=first_b, rules=("i",),
                  bias_kernel=_bias_kernel(layer))
    nw, nb = _launch(layer, x, d, want_bias=False)
    assert nb is None
    R.check_wgrad(f"wgrad {R.layer_id(layer)} without bias", nw, None, ref, row, centre_w=first_w, rules=("i",))
    R.check_wgrad(f"wgrad {R.layer_id(layer)} without bias", nw, None, ref, row)


# ----------------------------------------------------------------------------------------------------- e. CostRegNetWeightFn
NET_SHAPE = (2, 1, 8, 32, 96)       # 192, 32, 4 and 2 bricks per stride-1 launch at the four resolutions: runs of 4, then idle workgroups
NET_BOUND = 1e-4                    # the project's bound on a gradient of the whole network (tests/test_gpu_conv3d_bwd.py), of the tensor's scale
FROZEN = ("conv4.weight", "conv4.bias", "features.weight")


@functools.lru_cache(maxsize=None)
def _net():
    from uforecon_amd import cascade
    from uforecon_amd.scene import fill_state_dict

    m = cascade.CostRegNetWeight(1, 8)
    fill_state_dict(m, 23)              # no weight tensor near zero
    g = torch.Generator().manual_seed(24)
    B, _, D, H, W = NET_SHAPE
    return m, torch.randn(NET_SHAPE, generator=g), torch.randn(B, 8, D, H, W, generator=g), torch.randn(B, 1, D, H, W, generator=g)


def _loss(name):
    _, _, cf, cw = _net()
    both = lambda f, w: (f * cf.to(f)).sum() + (w * cw.to(w)).sum() + 0.1 * (f * f).mean()       # tests/test_gpu_conv3d_bwd.py's
    return {"both": both, "frozen": both, "no-x": both,
            "features": lambda f, w: (f * cf.to(f)).sum() + 0.1 * (f * f).mean(),
            "weights": lambda f, w: (w * cw.to(w)).sum(),
            "expanded": lambda f, w: f.sum()}[name]


@functools.lru_cache(maxsize=None)
def _cpu_gradients(name, dtype):
    m, x, _, _ = _net()
    return R.net_gradients(m, x, _loss(name), dtype, frozen=FROZEN if name == "frozen" else (), x_grad=name != "no-x")


@functools.lru_cache(maxsize=None)
def _hip_gradients(name):
    """{parameter: gradient, "x": d x} of the branch through unet3d.CostRegNetWeightFn, on a copy of the module"""
    m, x, _, _ = _net()
    m = copy.deepcopy(m).to(DEV)
    for k, p in m.named_parameters():
        p.requires_grad_(not (name == "frozen" and k in FROZEN))
    xh = x.to(DEV).requires_grad_(name != "no-x")
    f, w = m(xh)
    assert type(f.grad_fn).__name__.startswith("CostRegNetWeightFn")
    _loss(name)(f, w).backward()
    out = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()}
    out["x"] = None if xh.grad is None else xh.grad.detach().cpu()
    return out


def _check_net(name):
    got, r64, r32 = _hip_gradients(name), _cpu_gradients(name, torch.float64), _cpu_gradients(name, torch.float32)
    assert set(got) == set(r64)
    rows = []
    for k in got:
        assert (got[k] is None) == (r64[k] is None), k
        if got[k] is not None:
            assert got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all()), k
            rows.append((R.tensor_rel(got[k], r64[k]), R.tensor_rel(r32[k], r64[k]), k))
    for e, y, k in sorted(rows, reverse=True):
        print(f"MEASURE CostRegNetWeightFn {name} {NET_SHAPE} {k:16s}: kernels {e:.2e}  float32 torch autograd {y:.2e} of the tensor's scale "
              f"against float64 autograd  ({e / NET_BOUND:.2f} of the bound)")
    bad = {k: e for e, _, k in rows if not e < NET_BOUND}
    assert not bad, bad
    return got, r64, r32


def test_network_gradients_match_float64_autograd():
    got, _, _ = _check_net("both")
    assert all(v is not None for v in got.values()) and len(got) == 23


def test_network_loss_of_the_features_alone():
    """`d_wsig is None`: the weights head's cotangent is a zero tensor the backward makes itself"""
    got, r64, _ = _check_net("features")
    assert float(got["weights.weight"].abs().max()) == 0.0 and float(r64["weights.weight"].abs().max()) == 0.0


def test_network_loss_of_the_weights_alone():
    """`d_feat is None`: an all-zero cotangent (|max| 0) goes through the plane data-gradient kernel and the heads' kernel"""
    got, r64, _ = _check_net("weights")
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got["features.weight"].abs().max()) == 0.0 and float(r64["features.weight"].abs().max()) == 0.0


def test_network_expanded_cotangent():
    """`feat.sum()`: the cotangent arrives as a stride-0 expansion of one element"""
    _check_net("expanded")


def test_network_frozen_parameters():
    got, r64, r32 = _check_net("frozen")
    base = _hip_gradients("both")
    for k in FROZEN:
        assert got[k] is None
    for k, v in got.items():
        if v is not None:
            R.rows_close(f"{k} with {FROZEN} frozen", v, base[k], r64[k], r32[k])


def test_network_input_without_gradient():
    got, r64, r32 = _check_net("no-x")
    base = _hip_gradients("both")
    assert got["x"] is None
    for k, v in got.items():
        if v is not None:
            R.rows_close(f"{k} without d x", v, base[k], r64[k], r32[k])
