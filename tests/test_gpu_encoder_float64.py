"""The frame encoder's kernels (csrc/frustum.hip, fmt.hip, conv2d.hip, dcn.hip) against float64 restatements of the same
operations (tests/encoder_ref.py, pinned without a GPU by tests/test_encoder_ref.py), at the shapes the other tests skip: ragged
and empty runs of depth hypotheses, seven source views, 2 x 2 maps, token counts below one tile and above sixteen partial
states, token scales at which torch's own fp32 layer is no yardstick, workgroups that walk several groups of 256 pixels, one-row
and one-column images, taps exactly on the image border.

One acceptance rule, the one of tests/test_gpu_conv3d_planes.py (encoder_ref.accept):
    err(kernel, float64) < max(4 err(yardstick, float64), 1e-6),   errors relative to the float64 output's largest magnitude,
where the yardstick is the fp32 oracle or torch expression on the same inputs (for the FMT layer the careful fp32 expression,
see tests/test_fmt.py).  Both errors are printed."""
import copy

import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R
from oracle import dcn_oracle
from oracle import frustum_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------ correlate
@pytest.mark.parametrize("smooth", [True, False], ids=["band_limited", "white_noise"])
@pytest.mark.parametrize("name", list(R.CORRELATE_SHAPES))
def test_correlate_matches_float64(name, smooth):
    from uforecon_amd import frustum

    c = R.correlate_inputs(R.CORRELATE_SHAPES[name], smooth)
    runs, d_per = R.correlate_runs(c["C"], c["H"], c["W"], c["D"])
    print(f"{name}: {runs} runs of {d_per} hypotheses for D = {c['D']}, NS = {c['NS']}")
    ref = R.correlate64(c)
    yard_s, yard_a = FO.correlate(c["ref_fea"], c["src_feas"], c["ref_proj_pair"], c["src_proj_pairs"], c["depth_values"],
                                  c["view_weights"])
    run = lambda vw, want_sim=True: frustum.correlate(c["ref_fea"].to(DEV), torch.stack(c["src_feas"]).to(DEV), c["ref_proj_pair"],
                                                      c["src_proj_pairs"], c["depth_values"].to(DEV), vw, want_similarity=want_sim)
    vw = c["view_weights"].to(DEV)
    sim, agg = run(vw)
    sim_alone, none = run(None)
    assert none is None and torch.equal(sim_alone, sim)
    none, agg_alone = run(vw, want_sim=False)
    assert none is None and torch.equal(agg_alone, agg)           # the aggregate computed alone: bit for bit the same
    R.check_correlate(sim.cpu(), agg.cpu(), yard_s, yard_a, ref, f"{name} {'band-limited' if smooth else 'white noise'}")


# ------------------------------------------------------------------ FMT layer
@pytest.mark.parametrize("mode", R.FMT_MODES)
@pytest.mark.parametrize("case", R.FMT_CASES, ids=lambda c: "N%d_T%d_S%d_x%g" % c)
def test_fmt_layer_matches_float64(case, mode):
    from uforecon_amd import fmt

    p = R.fmt_params()
    x, src = R.fmt_tokens(*case, mode)
    with torch.no_grad():
        ref, yard = R.fmt_layer64(p, x, src), R.fmt_layer_careful32(p, x, src)
        got = fmt._layer(copy.deepcopy(p).to(DEV), x.to(DEV), None if src is None else src.to(DEV))
    R.accept(got.cpu(), yard, ref, f"fmt layer {case} {mode}")


# ------------------------------------------------------------------ pixel-wise view weights
@pytest.mark.parametrize("NS,D,H,W,gain", R.PIXELWISE_CASES)
def test_pixelwise_view_weights_match_float64(NS, D, H, W, gain):
    from uforecon_amd import cascade, frustum
    from uforecon_amd.scene import fill_state_dict

    net = fill_state_dict(cascade.PixelwiseNet(), 4).eval()
    sim = R.pixelwise_sim(NS, D, H, W, gain)
    vw64, agg64 = R.pixelwise64(net, sim)
    with torch.no_grad():
        yard_vw = torch.cat([net(sim[i][None, None]) for i in range(NS)], dim=1)[0]
        yard_agg = FO.aggregate_views(sim, yard_vw)
        vw, agg = frustum.view_weights(copy.deepcopy(net).to(DEV), sim.to(DEV))
    R.accept(vw.cpu(), yard_vw, vw64, f"pixel-wise weights {(NS, D, H, W)} x{gain:g}")
    R.accept(agg.cpu(), yard_agg, agg64, f"their aggregate {(NS, D, H, W)} x{gain:g}")


# ------------------------------------------------------------------ conv2d
def _conv2d_both(cin, cout, k, stride, B, H, W, label, relu=True, use_scale=True, sigmoid_from=-1, out_planar=False, with_skip=False):
    from uforecon_amd import ops

    x, w, sc, sh, g = R.conv2d_inputs(cin, cout, k, B, H, W)
    sc = sc if use_scale else None
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    skip = torch.randn(B, cout, Ho // 2, Wo // 2, generator=g) if with_skip else None
    kw = dict(relu=relu, sigmoid_from=sigmoid_from, skip=skip, out_planar=out_planar)
    ref = R.conv2d64(x, w, stride, sc, sh, **kw)
    yard = R.conv2d64(x, w, stride, sc, sh, dtype=torch.float32, **kw)        # the torch expression in fp32
    stem = cin == 3
    got = ops.conv2d((x if stem else x.permute(0, 2, 3, 1).contiguous()).to(DEV), w.to(DEV), stride, None if sc is None else sc.to(DEV),
                     sh.to(DEV), relu=relu, skip=None if skip is None else skip.permute(0, 2, 3, 1).contiguous().to(DEV),
                     in_planar=stem, out_planar=out_planar, sigmoid_from=sigmoid_from)
    R.accept(got.cpu(), yard, ref, label)
    return Ho * Wo


@pytest.mark.parametrize("cin,cout,k,stride,B,H,W,opts", [
    (8, 8, 3, 1, 1, 520, 512, {}),                                                    # 1040 groups > 1024 workgroups
    (8, 8, 3, 1, 64, 80, 128, {}),                                                    # 40 groups on 32 workgroups per image
    (32, 27, 3, 1, 64, 80, 128, dict(relu=False, use_scale=False, sigmoid_from=18, out_planar=True)),   # offsets | sigmoid(masks)
    (16, 32, 5, 2, 56, 160, 256, {}),                                                 # 40 groups on 37
    (16, 32, 1, 1, 64, 80, 128, dict(relu=False, use_scale=False, with_skip=True)),   # the lateral connection
], ids=["8to8_1x520x512", "8to8_64x80x128", "32to27_planar_sigmoid", "16to32_5x5_s2", "16to32_1x1_skip"])
def test_conv2d_workgroups_walking_several_pixel_groups(cin, cout, k, stride, B, H, W, opts):
    """conv2d_mfma_kernel's loop `for (grp = blockIdx.x; grp < n_groups; grp += gridDim.x)` iterating more than once -- what every
    stage-3 convolution of a 512 x 640 frame does (B = 3: 1280 groups on 683 workgroups)."""
    n_pixels = _conv2d_both(cin, cout, k, stride, B, H, W, f"conv2d {cin}->{cout} k{k} s{stride} B{B} {H}x{W}", **opts)
    blocks, n_groups = R.conv2d_launch(B, n_pixels)
    assert blocks < n_groups, (blocks, n_groups)       # launch_conv2d_t restated: a later change of the launch cannot un-test the path


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 1)])
@pytest.mark.parametrize("cin,cout,k,stride", R.CONV2D_LAYERS)
def test_conv2d_tiny_extents(cin, cout, k, stride, H, W):
    _conv2d_both(cin, cout, k, stride, 2, H, W, f"conv2d {cin}->{cout} k{k} s{stride} {H}x{W}")
    if cin != 3:                                                                      # (the stem writes channel-last only)
        _conv2d_both(cin, cout, k, stride, 2, H, W, f"conv2d {cin}->{cout} k{k} s{stride} {H}x{W} planar, no epilogue", relu=False,
                     use_scale=False, out_planar=True)


# ------------------------------------------------------------------ upsample_add
@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (3, 1), (17, 23)])
def test_upsample_add_matches_float64(C, h, w):
    """h = 1 / w = 1: the y1 / x1 clamp taken on every row / column."""
    from uforecon_amd import ops

    r, fine = R.upsample_inputs(2, C, h, w)
    yard = (F.interpolate(r.permute(0, 3, 1, 2), size=(2 * h, 2 * w), mode="bilinear") + fine).permute(0, 2, 3, 1)
    R.accept(ops.upsample_add(r.to(DEV), fine.to(DEV)).cpu(), yard, R.upsample_add64(r, fine), f"upsample_add C {C} {h}x{w}")


# ------------------------------------------------------------------ deformable convolution
@pytest.mark.parametrize("C,Cout", [(32, 32), (32, 16), (8, 8)])
@pytest.mark.parametrize("H,W", [(1, 37), (33, 1), (5, 7)])
def test_deform_conv2d_matches_float64(C, Cout, H, W):
    """One-row and one-column images, three images whose pixel count is no multiple of 64, taps exactly on -1, 0, H - 1, H, W and
    offsets of 1e6; with the mask and without.  No exclusions: the operation is continuous in the offsets."""
    from uforecon_amd import featurenet as FN
    from uforecon_amd import ops

    B = 3
    x, off, mask, w, bias = R.dcn_inputs(B, C, Cout, H, W)
    d = lambda t: None if t is None else t.double()
    dev = lambda t: None if t is None else t.to(DEV)
    for m, b in ((mask, bias), (None, None)):
        ref = dcn_oracle.deform_conv2d(d(x), d(off), d(w), d(b), 1, 1, 1, d(m))
        yard = dcn_oracle.deform_conv2d(x, off, w, b, 1, 1, 1, m)
        got = FN.deform_conv2d(dev(x), dev(off), dev(w), dev(b), 1, 1, 1, mask=dev(m))
        R.accept(got.cpu(), yard, ref, f"deform_conv2d {C}->{Cout} {H}x{W} mask {m is not None}")
    x_cl, om = dev(x.permute(0, 2, 3, 1).contiguous()), dev(torch.cat((off, mask), dim=1))
    if C != 32:       # the channel-last entry point exists for the 32-channel layers of FeatureNet only
        with pytest.raises(ops.UfrError):
            ops.deform_conv2d_cl(x_cl, om, dev(w), dev(bias))
        return
    ref = dcn_oracle.deform_conv2d(d(x), d(off), d(w), d(bias), 1, 1, 1, d(mask))
    yard = dcn_oracle.deform_conv2d(x, off, w, bias, 1, 1, 1, mask)
    R.accept(ops.deform_conv2d_cl(x_cl, om, dev(w), dev(bias)).cpu(), yard.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1),
             f"deform_conv2d_cl {C}->{Cout} {H}x{W}")
    g = torch.Generator().manual_seed(H + W)
    sc, sh = 0.5 + torch.rand(Cout, generator=g), torch.randn(Cout, generator=g)
    ep = lambda t: F.relu(t * sc.to(t.dtype)[None, :, None, None] + sh.to(t.dtype)[None, :, None, None])
    R.accept(ops.deform_conv2d_cl(x_cl, om, dev(w), dev(bias), dev(sc), dev(sh), relu=True, out_planar=True).cpu(), ep(yard), ep(ref),
             f"deform_conv2d_cl {C}->{Cout} {H}x{W} BatchNorm + ReLU, planar")
