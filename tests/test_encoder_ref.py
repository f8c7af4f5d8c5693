"""tests/encoder_ref.py pinned, without a GPU: each float64 restatement against the fp32 oracle / torch expression / golden vector
of the same operation, to the distance fp32 arithmetic explains, and the comparisons of tests/test_gpu_encoder_float64.py run
with the fp32 oracle standing in for the kernel (they pass) and with deliberately wrong stand-ins (each must fail).

The table above a test holds the distances MEASURED on the build host, each relative to the float64 output's largest magnitude;
`_pin` prints the distance and asserts it against the table's figure x 4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R
from oracle import dcn_oracle, fmt_oracle
from oracle import frustum_oracle as FO

HERE = os.path.dirname(os.path.abspath(__file__))

CORRELATE_SHAPES, FMT_CASES, PIXELWISE_CASES = R.CORRELATE_SHAPES, R.FMT_CASES, R.PIXELWISE_CASES

ULP32 = 2.0 ** -23          # a distance below one fp32 ulp of the output scale is not resolved: the floor of a measured figure


def _pin(table, label, value):
    print(f"{label}: {value:.2e} (measured {table[label]:.1e})")
    assert value <= 4 * max(table[label], ULP32), f"{label}: {value:.2e} > 4 x {table[label]:.1e}"


def _fo(c, with_weights=True):
    return FO.correlate(c["ref_fea"], c["src_feas"], c["ref_proj_pair"], c["src_proj_pairs"], c["depth_values"],
                        c["view_weights"] if with_weights else None)


# ------------------------------------------------------------------ correlate
M_GOLDEN = {
    "stage1_small similarity": 1.9e-05,
    "stage1_small aggregate": 2.3e-05,
    "stage3_small similarity": 3.7e-05,
    "stage3_small aggregate": 3.2e-05,
    "nv5_stage2 similarity": 1.6e-05,
    "nv5_stage2 aggregate": 9.5e-06,
    "edge similarity": 9.4e-06,
    "edge aggregate": 8.4e-06,
}


@pytest.mark.parametrize("name", ["stage1_small", "stage3_small", "nv5_stage2", "edge"])
def test_correlate64_agrees_with_the_references_golden_vectors(name):
    """The goldens are outputs of the reference itself, in fp32 on white-noise features: float64 stands that far from them."""
    c = R.correlate_inputs(name, smooth=False)
    g = np.load(os.path.join(HERE, "golden", f"correlate_{name}.npz"))
    r = R.correlate64(c)
    keep, zero_keep = R.correlate_masks(r, c["H"], c["W"])
    gs, ga = torch.from_numpy(g["similarity"]), torch.from_numpy(g["aggregated"])
    _pin(M_GOLDEN, f"{name} similarity", R.rel_err(gs, r["sim"], keep))
    _pin(M_GOLDEN, f"{name} aggregate", R.rel_err(ga, r["agg"], keep.all(0)))
    assert not bool((((gs == 0) != (r["sim"] == 0)) & zero_keep).any())
    assert 1.0 - float(zero_keep.double().mean()) <= R.MAX_EXCLUDED


M_CORRELATE = {
    "ragged_runs band-limited: oracle to float64": 1.4e-06,
    "ragged_runs band-limited: fp32 restatement to float64": 4.6e-06,
    "ragged_runs white noise: oracle to float64": 2.9e-06,
    "ragged_runs white noise: fp32 restatement to float64": 3.2e-06,
    "empty_run_edge band-limited: oracle to float64": 4.4e-06,
    "empty_run_edge band-limited: fp32 restatement to float64": 4.5e-06,
    "empty_run_edge white noise: oracle to float64": 1.1e-05,
    "empty_run_edge white noise: fp32 restatement to float64": 7.9e-06,
    "seven_views band-limited: oracle to float64": 6.8e-06,
    "seven_views band-limited: fp32 restatement to float64": 3.1e-06,
    "seven_views white noise: oracle to float64": 1.1e-05,
    "seven_views white noise: fp32 restatement to float64": 7.8e-06,
    "two_by_two band-limited: oracle to float64": 1.7e-07,
    "two_by_two band-limited: fp32 restatement to float64": 1.2e-07,
    "two_by_two white noise: oracle to float64": 5.5e-07,
    "two_by_two white noise: fp32 restatement to float64": 4.0e-07,
    "c64 band-limited: oracle to float64": 9.4e-07,
    "c64 band-limited: fp32 restatement to float64": 1.1e-06,
    "c64 white noise: oracle to float64": 3.1e-06,
    "c64 white noise: fp32 restatement to float64": 3.3e-06,
}


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("name", list(CORRELATE_SHAPES))
def test_correlate_comparison_accepts_the_oracle_and_pins_its_distance(name, smooth):
    """The GPU test's comparison with the fp32 oracle as the kernel and the fp32 restatement as the yardstick, and the other way
    round; the oracle's distance from float64 on band-limited and on white-noise features; the shares the check rests on."""
    c = R.correlate_inputs(CORRELATE_SHAPES[name], smooth)
    r = R.correlate64(c)
    sims, agg = _fo(c)
    r32 = R.correlate(c, torch.float32)
    kind = "band-limited" if smooth else "white noise"
    out = R.check_correlate(sims, agg, r32["sim"], r32["agg"], r, f"{name} {kind}, oracle as kernel")
    R.check_correlate(r32["sim"], r32["agg"], sims, agg, r, f"{name} {kind}, restatement as kernel")
    _pin(M_CORRELATE, f"{name} {kind}: oracle to float64", out["sim"][0])
    _pin(M_CORRELATE, f"{name} {kind}: fp32 restatement to float64", out["sim"][1])
    if name == "two_by_two":     # four elements, and the geometry (not the seed) puts all four footprints inside the source image
        assert out["zeros"] == 0.0 and out["excluded"] == 0.0
    else:                        # the zero-set check is not vacuous, and neither is the value check
        assert 0.04 <= out["zeros"] <= 0.7, out


@pytest.mark.parametrize("name", list(CORRELATE_SHAPES))
def test_correlate_comparison_rejects_wrong_kernels(name):
    over = CORRELATE_SHAPES[name]
    c = R.correlate_inputs(over, smooth=True)
    r = R.correlate64(c)
    sims, agg = _fo(c)
    # the last run of hypotheses never written (the kernel's outputs are torch.empty: whatever was there; here zeros and ones)
    runs, d_per = R.correlate_runs(over["C"], over["H"], over["W"], over["D"])
    last = min((runs - 1) * d_per, over["D"] - 1)
    for stale in (0.0, 1.0):
        bad_s, bad_a = sims.clone(), agg.clone()
        bad_s[:, last:], bad_a[last:] = stale, stale
        with pytest.raises(AssertionError):
            R.check_correlate(bad_s, bad_a, sims, agg, r, f"{name} last run dropped")
        with pytest.raises(AssertionError):          # ... in the aggregate alone
            R.check_correlate(sims, bad_a, sims, agg, r, f"{name} last run of the aggregate dropped")
    w = R.correlate(c, torch.float32, swap_corners=True)
    with pytest.raises(AssertionError):
        R.check_correlate(w["sim"], w["agg"], sims, agg, r, f"{name} corner weights swapped")


def test_correlate_run_split_of_the_cases():
    """The cases exist for these splits (launch_correlate, restated): ragged 5 + 4, an EMPTY sixth run, one run."""
    assert R.correlate_runs(4, 9, 13, 9) == (2, 5)
    assert R.correlate_runs(8, 20, 28, 25) == (6, 5) and 5 * 5 >= 25
    assert R.correlate_runs(16, 17, 23, 13) == (3, 5)
    assert R.correlate_runs(32, 2, 2, 1) == (1, 1) and R.correlate_runs(64, 8, 10, 5) == (1, 5)


# ------------------------------------------------------------------ FMT layer
M_FMT = {
    "(1, 1, 1, 1.0) self: careful fp32 to float64": 1.6e-07,
    "(1, 1, 1, 1.0) self: restatement with elu + 1 to the oracle": 0.0,
    "(1, 1, 1, 1.0) self_long: careful fp32 to float64": 1.4e-07,
    "(1, 1, 1, 1.0) self_long: restatement with elu + 1 to the oracle": 0.0,
    "(1, 1, 1, 1.0) cross: careful fp32 to float64": 2.1e-07,
    "(1, 1, 1, 1.0) cross: restatement with elu + 1 to the oracle": 0.0,
    "(2, 63, 257, 1.0) self: careful fp32 to float64": 3.2e-07,
    "(2, 63, 257, 1.0) self: restatement with elu + 1 to the oracle": 0.0,
    "(2, 63, 257, 1.0) self_long: careful fp32 to float64": 2.5e-07,
    "(2, 63, 257, 1.0) self_long: restatement with elu + 1 to the oracle": 2.4e-07,
    "(2, 63, 257, 1.0) cross: careful fp32 to float64": 3.1e-07,
    "(2, 63, 257, 1.0) cross: restatement with elu + 1 to the oracle": 0.0,
    "(1, 65, 1024, 8.0) self: careful fp32 to float64": 3.8e-07,
    "(1, 65, 1024, 8.0) self: restatement with elu + 1 to the oracle": 0.0,
    "(1, 65, 1024, 8.0) self_long: careful fp32 to float64": 2.4e-07,
    "(1, 65, 1024, 8.0) self_long: restatement with elu + 1 to the oracle": 2.2e-07,
    "(1, 65, 1024, 8.0) cross: careful fp32 to float64": 2.7e-07,
    "(1, 65, 1024, 8.0) cross: restatement with elu + 1 to the oracle": 0.0,
    "(1, 64, 256, 30.0) self: careful fp32 to float64": 2.4e-07,
    "(1, 64, 256, 30.0) self: restatement with elu + 1 to the oracle": 0.0,
    "(1, 64, 256, 30.0) self_long: careful fp32 to float64": 3.5e-07,
    "(1, 64, 256, 30.0) self_long: restatement with elu + 1 to the oracle": 2.0e-07,
    "(1, 64, 256, 30.0) cross: careful fp32 to float64": 3.4e-07,
    "(1, 64, 256, 30.0) cross: restatement with elu + 1 to the oracle": 0.0,
    "(2, 300, 255, 0.01) self: careful fp32 to float64": 3.2e-07,
    "(2, 300, 255, 0.01) self: restatement with elu + 1 to the oracle": 3.3e-07,
    "(2, 300, 255, 0.01) self_long: careful fp32 to float64": 2.8e-07,
    "(2, 300, 255, 0.01) self_long: restatement with elu + 1 to the oracle": 2.2e-07,
    "(2, 300, 255, 0.01) cross: careful fp32 to float64": 3.4e-07,
    "(2, 300, 255, 0.01) cross: restatement with elu + 1 to the oracle": 3.3e-07,
    "(1, 256, 4097, 3.0) self: careful fp32 to float64": 2.7e-07,
    "(1, 256, 4097, 3.0) self: restatement with elu + 1 to the oracle": 2.4e-07,
    "(1, 256, 4097, 3.0) self_long: careful fp32 to float64": 2.9e-07,
    "(1, 256, 4097, 3.0) self_long: restatement with elu + 1 to the oracle": 2.6e-07,
    "(1, 256, 4097, 3.0) cross: careful fp32 to float64": 2.1e-07,
    "(1, 256, 4097, 3.0) cross: restatement with elu + 1 to the oracle": 1.8e-07,
}


@pytest.mark.parametrize("mode", R.FMT_MODES)
@pytest.mark.parametrize("case", FMT_CASES)
def test_fmt_careful32_is_what_fp32_can_achieve(case, mode):
    p = R.fmt_params()
    x, src = R.fmt_tokens(*case, mode)
    with torch.no_grad():
        ref = R.fmt_layer64(p, x, src)
        c32 = R.fmt_layer_careful32(p, x, src)
        same = R.fmt_layer(p, x, src, torch.float32, phi=lambda t: F.elu(t) + 1)     # the oracle's expression, restated
        want = fmt_oracle.layer(p, x, src)
    _pin(M_FMT, f"{case} {mode}: careful fp32 to float64", R.rel_err(c32, ref))
    # same feature map, same precision: the restatement IS the oracle's layer, up to the order of its sums
    _pin(M_FMT, f"{case} {mode}: restatement with elu + 1 to the oracle", R.rel_err(same, want.double()))
    R.accept(c32, c32, ref, f"{case} {mode} careful32 as kernel")


M_ELU = {
    "scale 1.0 self: torch fp32": 2.7e-07,
    "scale 1.0 self: careful fp32": 3.2e-07,
    "scale 1.0 self: float64 elu + 1": 5.5e-16,
    "scale 1.0 self_long: torch fp32": 2.7e-07,
    "scale 1.0 self_long: careful fp32": 2.5e-07,
    "scale 1.0 self_long: float64 elu + 1": 4.6e-16,
    "scale 1.0 cross: torch fp32": 3.1e-07,
    "scale 1.0 cross: careful fp32": 3.1e-07,
    "scale 1.0 cross: float64 elu + 1": 4.0e-16,
    "scale 8.0 self: torch fp32": 2.5e-04,
    "scale 8.0 self: careful fp32": 3.8e-07,
    "scale 8.0 self: float64 elu + 1": 1.3e-12,
    "scale 8.0 self_long: torch fp32": 1.5e-01,
    "scale 8.0 self_long: careful fp32": 2.4e-07,
    "scale 8.0 self_long: float64 elu + 1": 1.1e-08,
    "scale 8.0 cross: torch fp32": 1.4e-04,
    "scale 8.0 cross: careful fp32": 2.7e-07,
    "scale 8.0 cross: float64 elu + 1": 7.1e-13,
    "scale 30.0 self: torch fp32": 1.9e-01,
    "scale 30.0 self: careful fp32": 2.4e-07,
    "scale 30.0 self: float64 elu + 1": 8.6e-09,
    "scale 30.0 self_long: torch fp32": 1.9e-01,
    "scale 30.0 self_long: careful fp32": 3.5e-07,
    "scale 30.0 self_long: float64 elu + 1": 8.3e-08,
    "scale 30.0 cross: torch fp32": 2.9e-01,
    "scale 30.0 cross: careful fp32": 3.4e-07,
    "scale 30.0 cross: float64 elu + 1": 4.2e-08,
}


def test_torchs_fp32_elu_plus_one_is_no_yardstick_away_from_unit_scale():
    """F.elu(t) + 1 is (exp(t) - 1) + 1: phi of a strongly negative t rounds to a multiple of 2^-24 or to zero, and a token whose
    four query features of a head are all strongly negative gets a message made of rounding.  At unit scale torch's layer is at
    fp32 rounding from float64; at token scale 8 (self-attention over 1024 tokens) it is more than 1e-2 away, where the careful
    expression stays at rounding.  At scale 30 even float64 elu + 1 is measurably not the mathematical layer."""
    p = R.fmt_params()
    fig = {}
    with torch.no_grad():
        for case in [(2, 63, 257, 1.0), (1, 65, 1024, 8.0), (1, 64, 256, 30.0)]:
            for mode in R.FMT_MODES:
                x, src = R.fmt_tokens(*case, mode)
                ref = R.fmt_layer64(p, x, src)
                fig[case[3], mode] = (R.rel_err(fmt_oracle.layer(p, x, src), ref), R.rel_err(R.fmt_layer_careful32(p, x, src), ref),
                                      R.rel_err(R.fmt_layer(p, x, src, torch.float64, phi=lambda t: F.elu(t) + 1), ref))
                print(f"scale {case[3]} {mode}: torch fp32 {fig[case[3], mode][0]:.2e}, careful fp32 {fig[case[3], mode][1]:.2e}, "
                      f"float64 elu + 1 {fig[case[3], mode][2]:.2e} from float64")
    for (scale, mode), (torch32, careful32, elu64) in fig.items():
        # (where elu + 1 has lost its small values the distance is made of which way single roundings fell: recorded, not bounded)
        print(f"scale {scale} {mode}: torch fp32 measured {M_ELU[f'scale {scale} {mode}: torch fp32']:.1e}, float64 elu + 1 "
              f"{M_ELU[f'scale {scale} {mode}: float64 elu + 1']:.1e}")
        if scale == 1.0:
            _pin(M_ELU, f"scale {scale} {mode}: torch fp32", torch32)
        _pin(M_ELU, f"scale {scale} {mode}: careful fp32", careful32)
    assert fig[8.0, "self_long"][0] > 1e-2 and fig[30.0, "self"][0] > 1e-2 and fig[30.0, "cross"][0] > 1e-2
    assert max(v[0] for (scale, _), v in fig.items() if scale == 1.0) < 1e-6 and max(v[1] for v in fig.values()) < 1e-6
    assert fig[30.0, "self_long"][2] > 1e-9


def test_fmt_comparison_rejects_a_head_reading_its_neighbours_state():
    p = R.fmt_params()
    with torch.no_grad():
        for case in FMT_CASES[1:]:
            for mode in R.FMT_MODES:
                x, src = R.fmt_tokens(*case, mode)
                ref, yard = R.fmt_layer64(p, x, src), R.fmt_layer_careful32(p, x, src)
                for h in (0, 6):
                    with pytest.raises(AssertionError):
                        R.accept(R.fmt_layer(p, x, src, torch.float32, wrong_head=h), yard, ref, f"{case} {mode} head {h} wrong")


# ------------------------------------------------------------------ pixel-wise weights
M_PIXELWISE = {
    "(7, 1, 3, 5) view weights": 1.2e-07,
    "(7, 1, 3, 5) aggregate": 1.7e-07,
    "(1, 48, 1, 1) view weights": 4.4e-08,
    "(1, 48, 1, 1) aggregate": 6.5e-08,
    "(3, 8, 17, 23) view weights": 5.4e-08,
    "(3, 8, 17, 23) aggregate": 1.2e-07,
}


@pytest.mark.parametrize("NS,D,H,W,gain", PIXELWISE_CASES)
def test_pixelwise64_agrees_with_the_module(NS, D, H, W, gain):
    from uforecon_amd import cascade
    from uforecon_amd.scene import fill_state_dict

    net = fill_state_dict(cascade.PixelwiseNet(), 4).eval()
    sim = R.pixelwise_sim(NS, D, H, W, gain)
    vw64, agg64 = R.pixelwise64(net, sim)
    with torch.no_grad():
        vw = torch.cat([net(sim[i][None, None]) for i in range(NS)], dim=1)[0]
    agg = FO.aggregate_views(sim, vw)
    _pin(M_PIXELWISE, f"{(NS, D, H, W)} view weights", R.rel_err(vw, vw64))
    _pin(M_PIXELWISE, f"{(NS, D, H, W)} aggregate", R.rel_err(agg, agg64))
    if gain > 1:
        o = R.pixelwise_logits64(net, sim)
        assert float((o.abs() > 17).double().mean()) > 0.2                # saturated sigmoids (1 - sigmoid(17) < 2^-24) are the case
    R.accept(vw, vw, vw64, "module as kernel")
    if D > 1:
        with pytest.raises(AssertionError):                             # a kernel that reads the first hypothesis only
            R.accept(R.pixelwise64(net, sim[:, :1])[0].float(), vw, vw64, "first hypothesis only")


# ------------------------------------------------------------------ conv2d, upsample_add
def _conv_expr32(x, w, stride, scale, shift, relu):
    """the fp32 expression of tests/test_gpu_conv2d.py"""
    y = F.conv2d(x, w, None, stride, w.shape[-1] // 2) * scale[None, :, None, None] + shift[None, :, None, None]
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


M_CONV2D = {
    "8->8 k3 s1 1x1": 9.1e-09,
    "8->8 k3 s1 2x3": 1.4e-07,
    "8->8 k3 s1 5x1": 7.7e-08,
    "8->8 k3 s1 36x52": 3.0e-07,
    "8->16 k5 s2 1x1": 3.5e-08,
    "8->16 k5 s2 2x3": 8.6e-08,
    "8->16 k5 s2 5x1": 5.4e-08,
    "8->16 k5 s2 36x52": 3.2e-07,
    "16->16 k3 s1 1x1": 5.1e-08,
    "16->16 k3 s1 2x3": 2.5e-07,
    "16->16 k3 s1 5x1": 1.5e-07,
    "16->16 k3 s1 36x52": 4.2e-07,
    "16->32 k5 s2 1x1": 2.8e-08,
    "16->32 k5 s2 2x3": 1.0e-07,
    "16->32 k5 s2 5x1": 4.5e-08,
    "16->32 k5 s2 36x52": 6.4e-07,
    "32->32 k3 s1 1x1": 3.0e-08,
    "32->32 k3 s1 2x3": 1.9e-07,
    "32->32 k3 s1 5x1": 8.3e-08,
    "32->32 k3 s1 36x52": 3.3e-07,
    "32->27 k3 s1 1x1": 5.9e-08,
    "32->27 k3 s1 2x3": 2.4e-07,
    "32->27 k3 s1 5x1": 1.3e-07,
    "32->27 k3 s1 36x52": 2.9e-07,
    "32->32 k1 s1 1x1": 8.5e-08,
    "32->32 k1 s1 2x3": 1.1e-07,
    "32->32 k1 s1 5x1": 1.3e-07,
    "32->32 k1 s1 36x52": 1.6e-07,
    "16->32 k1 s1 1x1": 9.9e-08,
    "16->32 k1 s1 2x3": 8.7e-08,
    "16->32 k1 s1 5x1": 8.1e-08,
    "16->32 k1 s1 36x52": 1.3e-07,
    "8->32 k1 s1 1x1": 6.7e-08,
    "8->32 k1 s1 2x3": 5.2e-08,
    "8->32 k1 s1 5x1": 4.9e-08,
    "8->32 k1 s1 36x52": 1.2e-07,
    "32->16 k1 s1 1x1": 7.7e-08,
    "32->16 k1 s1 2x3": 7.0e-08,
    "32->16 k1 s1 5x1": 1.1e-07,
    "32->16 k1 s1 36x52": 1.9e-07,
    "16->8 k1 s1 1x1": 5.3e-08,
    "16->8 k1 s1 2x3": 4.9e-08,
    "16->8 k1 s1 5x1": 5.3e-08,
    "16->8 k1 s1 36x52": 1.7e-07,
    "3->8 k3 s1 1x1": 4.0e-08,
    "3->8 k3 s1 2x3": 3.0e-07,
    "3->8 k3 s1 5x1": 4.6e-08,
    "3->8 k3 s1 36x52": 1.8e-07,
}


@pytest.mark.parametrize("cin,cout,k,stride", R.CONV2D_LAYERS)
def test_conv2d64_agrees_with_the_fp32_expression(cin, cout, k, stride):
    for B, H, W in [(2, 1, 1), (2, 2, 3), (2, 5, 1), (1, 36, 52)]:
        x, w, sc, sh, _ = R.conv2d_inputs(cin, cout, k, B, H, W)
        ref = R.conv2d64(x, w, stride, sc, sh, relu=True)
        _pin(M_CONV2D, f"{cin}->{cout} k{k} s{stride} {H}x{W}", R.rel_err(_conv_expr32(x, w, stride, sc, sh, True), ref))


M_CONV2D_EPILOGUE = {
    "offsets | sigmoid(masks), planar": 2.5e-07,
    "lateral with the upsampled skip": 1.4e-07,
}


def test_conv2d64_epilogue_and_the_comparison_rejects_an_unwritten_pixel_group():
    B, H, W = 2, 24, 40                                                   # 960 pixels: four groups of 256
    x, w, _, sh, g = R.conv2d_inputs(32, 27, 3, B, H, W)
    ref = R.conv2d64(x, w, 1, None, sh, sigmoid_from=18, out_planar=True)
    y = F.conv2d(x, w, sh, 1, 1)
    y32 = torch.cat((y[:, :18], torch.sigmoid(y[:, 18:])), 1)
    _pin(M_CONV2D_EPILOGUE, "offsets | sigmoid(masks), planar", R.rel_err(y32, ref))
    R.accept(y32, y32, ref, "expression as kernel")
    bad = y32.clone()
    bad.reshape(B, 27, H * W)[1, :, 256:512] = 0.0
    with pytest.raises(AssertionError):
        R.accept(bad, y32, ref, "second pixel group left at zero")
    # the lateral connection: 1x1 + bias + nearest-2x skip, channel-last
    x, w, _, sh, g = R.conv2d_inputs(16, 32, 1, B, H, W)
    skip = torch.randn(B, 32, H // 2, W // 2, generator=g)
    ref = R.conv2d64(x, w, 1, None, sh, skip=skip)
    y32 = (F.interpolate(skip, scale_factor=2, mode="nearest") + F.conv2d(x, w, sh)).permute(0, 2, 3, 1).contiguous()
    _pin(M_CONV2D_EPILOGUE, "lateral with the upsampled skip", R.rel_err(y32, ref))
    bad = y32.clone()
    bad.reshape(B, H * W, 32)[0, 256:512] = 0.0
    with pytest.raises(AssertionError):
        R.accept(bad, y32, ref, "second pixel group left at zero")


def test_conv2d_launch_restated_for_the_multi_group_cases():
    """(B, output pixels) of the GPU file's multi-group cases really give fewer workgroups than groups, the largest shape of
    tests/test_gpu_conv2d.py does not, and the benchmark's stage-3 layers (B = 3, 512 x 640) do."""
    assert R.conv2d_launch(1, 520 * 512) == (1024, 1040)
    assert R.conv2d_launch(64, 80 * 128) == (32, 40) and R.conv2d_launch(56, 80 * 128) == (37, 40)
    assert R.conv2d_launch(2, 128 * 160) == (80, 80) and R.conv2d_launch(3, 512 * 640) == (683, 1280)


M_UPSAMPLE = {
    "C 8 1x1: torch fp32 to float64": 3.7e-08,
    "C 8 1x1: tap form fp32 to float64": 3.7e-08,
    "C 16 1x1: torch fp32 to float64": 3.4e-08,
    "C 16 1x1: tap form fp32 to float64": 3.4e-08,
    "C 8 1x5: torch fp32 to float64": 4.4e-08,
    "C 8 1x5: tap form fp32 to float64": 4.4e-08,
    "C 16 1x5: torch fp32 to float64": 6.0e-08,
    "C 16 1x5: tap form fp32 to float64": 6.0e-08,
    "C 8 3x1: torch fp32 to float64": 3.9e-08,
    "C 8 3x1: tap form fp32 to float64": 3.9e-08,
    "C 16 3x1: torch fp32 to float64": 5.8e-08,
    "C 16 3x1: tap form fp32 to float64": 5.8e-08,
    "C 8 17x23: torch fp32 to float64": 7.8e-08,
    "C 8 17x23: tap form fp32 to float64": 6.8e-08,
    "C 16 17x23: torch fp32 to float64": 5.7e-08,
    "C 16 17x23: tap form fp32 to float64": 6.5e-08,
}


@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (3, 1), (17, 23)])
def test_upsample_add64_and_the_comparison_rejects_an_unclamped_tap(C, h, w):
    r, fine = R.upsample_inputs(2, C, h, w)
    ref = R.upsample_add64(r, fine)
    y32 = (F.interpolate(r.permute(0, 3, 1, 2), size=(2 * h, 2 * w), mode="bilinear") + fine).permute(0, 2, 3, 1)
    taps = R.upsample_add_taps(r, fine)
    _pin(M_UPSAMPLE, f"C {C} {h}x{w}: torch fp32 to float64", R.rel_err(y32, ref))
    _pin(M_UPSAMPLE, f"C {C} {h}x{w}: tap form fp32 to float64", R.rel_err(taps, ref))
    R.accept(taps, y32, ref, "tap form as kernel")
    if h * w > 1:
        with pytest.raises(AssertionError):
            R.accept(R.upsample_add_taps(r, fine, clamp_x1=False), y32, ref, "x1 not clamped")


# ------------------------------------------------------------------ deformable convolution
M_DCN = {
    "C 32->32 1x37: fp32 oracle to float64": 4.2e-07,
    "C 32->32 1x37: fp32 oracle to float64, no mask": 1.4e-06,
    "C 32->16 1x37: fp32 oracle to float64": 6.0e-07,
    "C 32->16 1x37: fp32 oracle to float64, no mask": 1.6e-06,
    "C 8->8 1x37: fp32 oracle to float64": 5.3e-07,
    "C 8->8 1x37: fp32 oracle to float64, no mask": 1.5e-06,
    "C 32->32 33x1: fp32 oracle to float64": 5.1e-07,
    "C 32->32 33x1: fp32 oracle to float64, no mask": 1.1e-06,
    "C 32->16 33x1: fp32 oracle to float64": 3.3e-07,
    "C 32->16 33x1: fp32 oracle to float64, no mask": 1.1e-06,
    "C 8->8 33x1: fp32 oracle to float64": 3.1e-07,
    "C 8->8 33x1: fp32 oracle to float64, no mask": 8.0e-07,
    "C 32->32 5x7: fp32 oracle to float64": 1.8e-07,
    "C 32->32 5x7: fp32 oracle to float64, no mask": 5.4e-07,
    "C 32->16 5x7: fp32 oracle to float64": 1.6e-07,
    "C 32->16 5x7: fp32 oracle to float64, no mask": 4.7e-07,
    "C 8->8 5x7: fp32 oracle to float64": 1.2e-07,
    "C 8->8 5x7: fp32 oracle to float64, no mask": 2.7e-07,
}


@pytest.mark.parametrize("C,Cout", [(32, 32), (32, 16), (8, 8)])
@pytest.mark.parametrize("H,W", [(1, 37), (33, 1), (5, 7)])
def test_dcn_oracle_in_float64_and_the_inputs_sit_on_the_decisions(C, Cout, H, W):
    x, off, mask, w, bias = R.dcn_inputs(3, C, Cout, H, W)
    d = lambda *ts: [None if t is None else t.double() for t in ts]
    ref = dcn_oracle.deform_conv2d(*d(x, off, w, bias), 1, 1, 1, mask.double())
    y32 = dcn_oracle.deform_conv2d(x, off, w, bias, 1, 1, 1, mask)
    _pin(M_DCN, f"C {C}->{Cout} {H}x{W}: fp32 oracle to float64", R.rel_err(y32, ref))
    ref_n = dcn_oracle.deform_conv2d(*d(x, off, w, None), 1, 1, 1, None)
    _pin(M_DCN, f"C {C}->{Cout} {H}x{W}: fp32 oracle to float64, no mask",
         R.rel_err(dcn_oracle.deform_conv2d(x, off, w, None, 1, 1, 1, None), ref_n))
    ys = torch.arange(H).reshape(H, 1) - 1.0
    xs = torch.arange(W).reshape(1, W) - 1.0
    ty = torch.stack([ys + k // 3 + off[0, 2 * k] for k in range(9)])
    tx = torch.stack([xs + k % 3 + off[0, 2 * k + 1] for k in range(9)])
    for v in (-1.0, 0.0, H - 1.0, float(H)):
        assert bool((ty == v).any()), v
    for v in (-1.0, 0.0, W - 1.0, float(W)):
        assert bool((tx == v).any()), v
    assert float(off.abs().max()) == 1e6
    bad = y32.clone()
    bad[2, :, H - 1, W - 1] = 0.0                                          # the last pixel of the last image never stored
    with pytest.raises(AssertionError):
        R.accept(bad, y32, ref, "last pixel missing")
