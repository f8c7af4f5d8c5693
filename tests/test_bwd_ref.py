"""CPU self-tests of the float64 backward yardstick (tests/bwd_ref.py): the ReLU indirection changes nothing, the
float32 oracle's own gradients lie inside the envelope, the envelope is empty without ambiguous units, and a gradient
that is subtly wrong -- one element off by 1e-3 of itself, or two points' d_pv rows swapped -- fails the check."""
import pytest
import torch

import bwd_ref as R
from helpers import load_weights
from oracle import ufo_oracle as O

EPS_FP32 = 2e-5      # the float32 oracle against float64: an fp32-grade bound (measured worst 4e-6)
EPS = R.EPS          # the kernels' bound


def _case(NV=3, RN=3, SN=32, seed=3):
    x, rgb, mask, dirs = R.oracle_tokens(NV, RN, SN)
    g = torch.Generator().manual_seed(seed)
    co_rad = torch.rand(RN * SN, 3, generator=g) - 0.5
    co_srdf = torch.rand(RN, SN, generator=g) - 0.5
    return x, rgb, mask, dirs, co_rad, co_srdf


def _fp32_grads(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf):
    keys = R.VIEW_KEYS + R.RAY_KEYS
    Pg = {k: v.clone().requires_grad_(k in keys) for k, v in P.items()}
    xr = x.clone().requires_grad_(True)
    want = {}
    rad, srdf = O.aggregate_tokens(Pg, xr, rgb, mask, dirs, RN, SN, want=want)
    want["view_out"].retain_grad()
    ((rad * co_rad).sum() + (srdf * co_srdf).sum()).backward()
    g = {k: Pg[k].grad for k in keys}
    g["d_pv"] = xr.grad[:, :, 32:72].sum(1)
    g["d_token0"] = want["view_out"].grad[:, 0]
    return g


def test_relu_indirection_is_plain_relu():
    x = torch.randn(100, dtype=torch.float64)
    assert torch.equal(O._relu(x), torch.relu(x))


@pytest.mark.parametrize("NV", [2, 3, 6])
def test_fp32_oracle_lies_inside_the_envelope(NV):
    P = load_weights()
    RN, SN = 3, 32
    x, rgb, mask, dirs, co_rad, co_srdf = _case(NV, RN, SN)
    e = R.grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf)
    print(f"NV {NV}: |A| = {len(e.ambiguous)}")
    g = _fp32_grads(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf)
    ex = e.excesses(g)
    assert set(ex) == set(e.g_nom) - {R.SHIFT_BIAS}
    assert max(ex.values()) < EPS_FP32, ex
    assert e.check_shift_bias(g[R.SHIFT_BIAS])


def test_envelope_without_ambiguous_units_is_zero_and_flips_are_counted():
    P = load_weights()
    RN, SN = 3, 32
    x, rgb, mask, dirs, co_rad, co_srdf = _case()
    e0 = R.grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf, tau=0.0)
    assert e0.ambiguous == []
    assert all(float(v.abs().max()) == 0.0 for v in e0.env.values())
    # a wider tau takes in more units; each one widens the envelope where its flip moves a gradient, and nowhere else
    e1 = R.grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf, tau=1e-3, cap=10_000)
    assert len(e1.ambiguous) > 0
    assert sum(float(v.abs().max() > 0) for v in e1.env.values()) > 0
    for k in e0.g_nom:
        assert torch.equal(e0.g_nom[k], e1.g_nom[k]), k
    # the nominal gradient is the one of plain torch.relu
    g = _fp32_grads({k: v.double() for k, v in P.items()}, x.double(), rgb.double(), mask.double(), dirs.double(), RN, SN,
                    co_rad.double(), co_srdf.double())
    for k in e0.g_nom:
        assert float((g[k] - e0.g_nom[k]).abs().max()) <= 1e-12 * max(float(g[k].abs().max()), 1.0), k


def test_a_flip_inside_the_ambiguous_set_is_absorbed_and_caught_outside_it():
    """A float64 backward with one ambiguous unit's mask inverted -- what a kernel whose forward put that unit on the other
    side of zero computes -- lies inside the envelope at eps = 0, and outside the envelope of a yardstick that does not
    know the unit (tau = 0) by far more than EPS: flips are absorbed exactly, not by a looser bound."""
    P = load_weights()
    RN, SN = 3, 32
    x, rgb, mask, dirs, co_rad, co_srdf = _case()
    e = R.grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf, tau=1e-3, cap=10_000, keep_flips=True)
    e0 = R.grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf, tau=0.0)
    assert len(e.flipped) == len(e.ambiguous) > 0
    worst = max(e.flipped, key=lambda gf: max(e0.excesses(gf).values()))
    assert max(e.excesses(worst).values()) == 0.0
    assert max(e0.excesses(worst).values()) > 10 * EPS


@pytest.mark.parametrize("mutation", ["scale_weight_element", "swap_d_pv_rows"])
def test_mutated_gradients_fail_the_check(mutation):
    """The check would catch a subtly wrong kernel: starting from the float32 oracle's gradients (which pass), one weight
    gradient element scaled by 1 + 1e-3, or two points' d_pv rows swapped, fails at EPS."""
    P = load_weights()
    RN, SN = 3, 32
    x, rgb, mask, dirs, co_rad, co_srdf = _case()
    e = R.grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf)
    g = _fp32_grads(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf)
    assert max(e.excesses(g).values()) < EPS
    g = {k: v.clone() for k, v in g.items()}
    if mutation == "scale_weight_element":
        k = O.VT + "mlp.2.weight"
        room = (e.g_nom[k].abs() - e.env[k]).reshape(-1)
        i = int(room.argmax())                    # the largest element the envelope does not cover
        g[k].view(-1)[i] *= 1 + 1e-3
        bad = e.excesses(g)
        assert bad[k] > EPS, bad[k]
        assert all(v < EPS for n, v in bad.items() if n != k)
    else:
        d = g["d_pv"]
        norms = d.norm(dim=1)
        a, b = int(norms.argmax()), int(norms.argmin())
        d[[a, b]] = d[[b, a]]
        assert e.excess("d_pv", d) > EPS
