"""Float64 restatements of the frame encoder's operations (csrc/frustum.hip, fmt.hip, conv2d.hip, dcn.hip) and the acceptance
rule their GPU tests share.  Plain torch on the CPU, no product code: tests/test_encoder_ref.py pins these restatements against
the fp32 oracles, the torch expressions and the reference's golden vectors, and proves that the comparisons below reject wrong
kernels; tests/test_gpu_encoder_float64.py judges the kernels with them.

Every restatement takes a ``dtype``: float64 is the reference, float32 the same expression at the kernels' precision (used as a
stand-in for a kernel where no GPU is present, and -- with one of the ``wrong`` switches -- as a deliberately wrong kernel).

  correlate        homo_warping_trans + similarity + view aggregate   code1/encoder_utils/fmt/module.py:329-367, TransMVSNet.py:66-97
  fmt_layer        EncoderLayer / LinearAttention                     code1/encoder_utils/fmt/FMT.py:25-38, 99-113
  pixelwise64      PixelwiseNet + aggregate                           TransMVSNet.py:23-41, 80-97
  conv2d64         Conv2d / FPN laterals / DCN.conv_offset_mask       module.py:26-62, 388-468; dcn.py:66-70
  upsample_add     FMT_with_pathway._push_down's sum                  FMT.py:226-235
"""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F

HEADS = 8

# ------------------------------------------------------------------ the cases both test files use
CORRELATE_SHAPES = {
    "ragged_runs": dict(C=4, H=9, W=13, D=9, NV=2, seed=61),                        # runs of 5 + 4 hypotheses
    "empty_run_edge": dict(C=8, H=20, W=28, D=25, NV=3, seed=62, edge=True),         # an empty sixth run; behind the camera
    "seven_views": dict(C=16, H=17, W=23, D=13, NV=8, seed=63),                      # NS = UFR_MAX_VIEWS
    "two_by_two": dict(C=32, H=2, W=2, D=1, NV=2, seed=64),
    "c64": dict(C=64, H=8, W=10, D=5, NV=4, seed=65),
}
# (N, T, S, token scale): T < 64 and T = 1, S = 1, S an exact multiple of 256, ragged S, seventeen partial states (S = 4097)
FMT_CASES = [(1, 1, 1, 1.0), (2, 63, 257, 1.0), (1, 65, 1024, 8.0), (1, 64, 256, 30.0), (2, 300, 255, 0.01), (1, 256, 4097, 3.0)]
# (NS, D, H, W, gain on the similarity): NS = 7 with D = 1, one pixel, saturated sigmoids
PIXELWISE_CASES = [(7, 1, 3, 5, 1.0), (1, 48, 1, 1, 1.0), (3, 8, 17, 23, 50.0)]


# ------------------------------------------------------------------ the acceptance rule (tests/test_gpu_conv3d_planes.py)
def rel_err(a: torch.Tensor, ref: torch.Tensor, keep=None) -> float:
    """max |a - ref| over the kept elements, relative to the float64 output's largest magnitude."""
    d = (a.detach().double().cpu() - ref).abs()
    if keep is not None:
        d = d[keep]
    return float(d.max()) / max(float(ref.abs().max()), 1e-300) if d.numel() else 0.0


def accept(got, yardstick, ref, label: str, keep=None, slack: float = 0.0):
    """err(kernel, f64) < max(4 err(yardstick32, f64), 1e-6) [+ slack], errors relative to max |f64|.  ``slack`` is zero unless the
    caller derives one from the reference side or a documented property of an intrinsic.  Prints both errors; returns them."""
    assert tuple(got.shape) == tuple(ref.shape), f"{label}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite output"
    e_k, e_y = rel_err(got, ref, keep), rel_err(yardstick, ref, keep)
    print(f"{label}: kernel {e_k:.2e}  yardstick {e_y:.2e} of the output scale")
    assert e_k < max(4 * e_y, 1e-6) + slack, f"{label}: kernel {e_k:.2e} vs yardstick {e_y:.2e}"
    return e_k, e_y


# ------------------------------------------------------------------ correlation volume
def _fold(pp: torch.Tensor) -> torch.Tensor:
    out = pp[0].clone()
    out[:3, :4] = pp[1, :3, :3] @ pp[0, :3, :4]
    return out


def correlate_inputs(name_or_over, smooth: bool):
    """A seeded case of uforecon_amd.scene.make_correlate_case; ``smooth``: band-limited features (the 3x3 box filter twice), like
    real feature maps, instead of white noise."""
    from uforecon_amd.scene import F_avg, make_correlate_case

    c = make_correlate_case(name_or_over) if isinstance(name_or_over, str) else make_correlate_case("custom", **name_or_over)
    if smooth:
        c["ref_fea"] = F_avg(F_avg(c["ref_fea"]))
        c["src_feas"] = [F_avg(F_avg(t)) for t in c["src_feas"]]
    return c


def correlate(case, dtype=torch.float64, with_weights: bool = True, swap_corners: bool = False, rel_proj=None):
    """The case's inputs taken to ``dtype`` (projections included: the relative projection src @ inverse(ref) is formed in
    ``dtype`` from the projection pairs unless ``rel_proj`` (NS,12) is given) -> dict(sim (NS,D,H,W), agg (D,H,W) or None,
    px, py (NS,D,H,W): projected pixel coordinates, qz (NS,D,H,W): projected depth).  grid_sample(bilinear, zeros,
    align_corners=True) un-normalises x_n = px / ((W-1)/2) - 1 back to px, so the four corners are taken at px, py directly.
    ``swap_corners``: a wrong kernel that exchanges the weights of the north-east and south-west corners."""
    ref = case["ref_fea"].to(dtype)
    C, H, W = ref.shape
    depth = case["depth_values"].to(dtype)
    D = depth.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    xyz = torch.stack((xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=dtype)))            # (3, HW)
    ref_inv = torch.inverse(_fold(case["ref_proj_pair"].to(dtype)))
    sims, pxs, pys, qzs = [], [], [], []
    for i, (src, pp) in enumerate(zip(case["src_feas"], case["src_proj_pairs"])):
        proj = (_fold(pp.to(dtype)) @ ref_inv)[:3] if rel_proj is None else rel_proj[i].to(dtype).reshape(3, 4)
        q = (proj[:, :3] @ xyz).unsqueeze(1) * depth.reshape(1, D, H * W) + proj[:, 3].reshape(3, 1, 1)   # (3, D, HW)
        qz = q[2]
        invalid = qz < 1e-6
        px, py = q[0] / qz, q[1] / qz
        far_x, far_y = -98.0 * (W - 1) / 2, -98.0 * (H - 1) / 2                                     # x_n = y_n = -99
        px = torch.where(invalid, torch.full_like(px, far_x), px)
        py = torch.where(invalid, torch.full_like(py, far_y), py)
        sx = torch.nan_to_num(px, nan=-2.0).clamp(-2.0, W + 1.0)     # beyond these every corner is outside anyway
        sy = torch.nan_to_num(py, nan=-2.0).clamp(-2.0, H + 1.0)
        x0, y0 = torch.floor(sx), torch.floor(sy)
        wx, wy = sx - x0, sy - y0
        flat = src.to(dtype).reshape(C, H * W)

        def corner(yy, xx, wgt):
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().reshape(-1)
            return flat[:, idx].reshape(C, D, H * W) * (wgt * ok.to(dtype)).unsqueeze(0)

        w_nw, w_ne, w_sw, w_se = (1 - wy) * (1 - wx), (1 - wy) * wx, wy * (1 - wx), wy * wx
        if swap_corners:
            w_ne, w_sw = w_sw, w_ne
        warped = corner(y0, x0, w_nw) + corner(y0, x0 + 1, w_ne) + corner(y0 + 1, x0, w_sw) + corner(y0 + 1, x0 + 1, w_se)
        sims.append((warped * ref.reshape(C, 1, H * W)).mean(0).reshape(D, H, W))
        pxs.append(px.reshape(D, H, W))
        pys.append(py.reshape(D, H, W))
        qzs.append(qz.reshape(D, H, W))
    sim = torch.stack(sims)
    agg = None
    if with_weights:
        vw = case["view_weights"].to(dtype)
        s, w = torch.zeros_like(sim[0]), torch.full_like(vw[0], 1e-5)
        for i in range(sim.shape[0]):                                  # TransMVSNet.py:86-97: views in order, sums from 0 and 1e-5
            s = s + sim[i] * vw[i].unsqueeze(0)
            w = w + vw[i]
        agg = s / w.unsqueeze(0)
    return dict(sim=sim, agg=agg, px=torch.stack(pxs), py=torch.stack(pys), qz=torch.stack(qzs))


def correlate64(case, with_weights: bool = True):
    return correlate(case, torch.float64, with_weights)


MAX_EXCLUDED = 5e-3      # a condition on the cases, not a measurement: at most 0.5 % of a case may escape the comparison


def correlate_masks(ref64, H: int, W: int):
    """keep (NS,D,H,W): elements whose value is compared -- all but those within 1e-5 of the ONE discontinuous decision, qz < 1e-6
    (bilinear sampling with zero padding is continuous in the coordinates).  zero_keep: elements whose zero-ness is compared --
    those, less the ones whose projected coordinate lies within 1e-3 px of where the footprint enters the image (-1, W, H)."""
    keep = (ref64["qz"] - 1e-6).abs() >= 1e-5
    px, py = ref64["px"], ref64["py"]
    edge = ((px + 1).abs() < 1e-3) | ((px - W).abs() < 1e-3) | ((py + 1).abs() < 1e-3) | ((py - H).abs() < 1e-3)
    return keep, keep & ~edge


def check_correlate(got_sim, got_agg, yard_sim, yard_agg, ref64, label: str):
    """The comparison of the correlate GPU tests: values by the acceptance rule on the kept elements, the similarity's zero set
    equal to the float64 zero set, and the shares that make the check meaningful.  Returns the figures it printed."""
    NS, D, H, W = ref64["sim"].shape
    keep, zero_keep = correlate_masks(ref64, H, W)
    excluded = 1.0 - float(zero_keep.double().mean())
    zeros = float((ref64["sim"] == 0).double().mean())
    print(f"{label}: excluded {excluded:.2e} of the elements, zeros {zeros:.2f}")
    assert excluded <= MAX_EXCLUDED, f"{label}: {excluded:.2e} of the case is excluded"
    out = dict(excluded=excluded, zeros=zeros)
    out["sim"] = accept(got_sim, yard_sim, ref64["sim"], label + " similarity", keep)
    gz, rz = (got_sim.cpu() == 0), (ref64["sim"] == 0)
    bad = int(((gz != rz) & zero_keep).sum())
    assert bad == 0, f"{label}: {bad} elements are zero on one side only"
    if got_agg is not None:
        out["agg"] = accept(got_agg, yard_agg, ref64["agg"], label + " aggregate", keep.all(0))
    return out


def correlate_runs(C: int, H: int, W: int, D: int):
    """launch_correlate's split of the D hypotheses over gridDim.y, restated: (number of runs, hypotheses per run)."""
    threads = H * W * (C // 4)
    dsplit = max(1, min((8192 * 64 + threads - 1) // threads, D // 4))
    return dsplit, (D + dsplit - 1) // dsplit


# ------------------------------------------------------------------ FMT layer
def phi_careful(t: torch.Tensor) -> torch.Tensor:
    """elu(t) + 1 as mathematics has it: exp(t) for t <= 0 evaluated directly.  torch's F.elu(t) + 1 computes (exp(t) - 1) + 1,
    which rounds phi of a strongly negative t to a multiple of 2^-24 (fp32) or 2^-53 (float64) -- or to zero."""
    return torch.where(t > 0, t + 1, torch.exp(torch.clamp(t, max=0)))


def _heads(t):
    n, l, c = t.shape
    return t.reshape(n, l, HEADS, c // HEADS).permute(0, 2, 1, 3)                  # (N, H, L, 4)


def fmt_layer(p, x, src, dtype=torch.float64, phi=phi_careful, wrong_head=None):
    """oracle/fmt_oracle.py's layer at ``dtype`` with the feature map ``phi``; p: a uforecon_amd.fmt._LayerParams.
    ``wrong_head`` = h: a wrong kernel that reads head h + 1's state (KV and sum K) for head h."""
    P = lambda t: t.detach().to(dtype)
    a = p.attention
    x = x.to(dtype)
    kv = x if src is None else src.to(dtype)
    lin = lambda t, m: F.linear(t, P(m.weight), P(m.bias))
    q, k, v = _heads(phi(lin(x, a.query_projection))), _heads(phi(lin(kv, a.key_projection))), _heads(lin(kv, a.value_projection))
    state = k.transpose(2, 3) @ v                                                   # (N, H, 4, 4): sum_s phi(k)^T v
    ksum = k.sum(dim=2, keepdim=True)                                               # (N, H, 1, 4)
    if wrong_head is not None:
        state, ksum = state.clone(), ksum.clone()
        state[:, wrong_head], ksum[:, wrong_head] = state[:, wrong_head + 1], ksum[:, wrong_head + 1]
    msg = (q @ state) / ((q * ksum).sum(-1, keepdim=True) + 1e-6)                   # (N, H, T, 4)
    msg = msg.permute(0, 2, 1, 3).reshape(x.shape)
    x = F.layer_norm(x + lin(msg, a.out_projection), x.shape[-1:], P(p.norm1.weight), P(p.norm1.bias))
    y = lin(F.relu(lin(x, p.linear1)), p.linear2)
    return F.layer_norm(x + y, x.shape[-1:], P(p.norm2.weight), P(p.norm2.bias))


def fmt_layer64(params, x, src):
    return fmt_layer(params, x, src, torch.float64)


def fmt_layer_careful32(params, x, src):
    """What fp32 arithmetic can achieve on this layer: the yardstick of the kernel."""
    return fmt_layer(params, x, src, torch.float32)


def fmt_params(seed: int = 3):
    """The parameters of tests/test_fmt.py::test_fmt_layer_kernel_matches_the_torch_layer."""
    from uforecon_amd import fmt

    torch.manual_seed(seed)
    p = fmt._LayerParams(32)
    with torch.no_grad():
        for q in p.parameters():
            q.copy_(torch.randn(q.shape) * (0.3 if q.dim() > 1 else 0.1))
        p.norm1.weight.add_(1.0)
        p.norm2.weight.add_(1.0)
    return p


FMT_MODES = ("self", "self_long", "cross")


def fmt_tokens(N: int, T: int, S: int, scale: float, mode: str):
    """Tokens of an (N, T, S, scale) case: "cross": x (N,T,32) attends to src (N,S,32); "self": x (N,T,32) alone; "self_long":
    self-attention over the S tokens (the state kernel's paths -- ragged blocks, many partial states -- in self-attention too)."""
    g = torch.Generator().manual_seed(1000 * T + S)
    x = torch.randn(N, T, 32, generator=g) * scale
    src = torch.randn(N, S, 32, generator=g) * scale
    return {"self": (x, None), "self_long": (src, None), "cross": (x, src)}[mode]


# ------------------------------------------------------------------ pixel-wise view weights
def pixelwise64(net, sim):
    """PixelwiseNet.double() on every view's volume (max over D of the sigmoid) and the aggregate in the reference's order:
    sim (NS,D,H,W) -> view weights (NS,H,W), aggregated (D,H,W), both float64."""
    net64 = copy.deepcopy(net).cpu().double().eval()
    sim = sim.detach().cpu().double()
    with torch.no_grad():
        vw = torch.cat([net64(sim[i][None, None]) for i in range(sim.shape[0])], dim=1)[0]
    s, w = torch.zeros_like(sim[0]), torch.full_like(vw[0], 1e-5)
    for i in range(sim.shape[0]):
        s = s + sim[i] * vw[i].unsqueeze(0)
        w = w + vw[i]
    return vw, s / w.unsqueeze(0)


def pixelwise_logits64(net, sim):
    """conv2(conv1(conv0(.))) of PixelwiseNet in float64, before the sigmoid: (NS,D,H,W)."""
    net64 = copy.deepcopy(net).cpu().double().eval()
    with torch.no_grad():
        return net64.conv2(net64.conv1(net64.conv0(sim.detach().cpu().double().unsqueeze(1)))).squeeze(1)


def pixelwise_sim(NS: int, D: int, H: int, W: int, gain: float = 1.0):
    return (torch.rand(NS, D, H, W, generator=torch.Generator().manual_seed(NS)) * 2 - 0.5) * gain


# ------------------------------------------------------------------ plain convolutions and the pathway's sum
def conv2d64(x, w, stride=1, scale=None, shift=None, relu=False, sigmoid_from=-1, skip=None, out_planar=False,
             dtype=torch.float64):
    """F.conv2d (zero padding k // 2) at ``dtype`` with ufr_conv2d's epilogue: out = [relu](conv * scale + shift), sigmoid on the
    channels >= sigmoid_from, + the nearest-2x-upsampled skip.  x (B,cin,H,W) planar, skip (B,cout,Ho/2,Wo/2) planar; returns
    the kernel's layout: channel-last (B,Ho,Wo,cout) or, with ``out_planar``, (B,cout,Ho,Wo)."""
    t = lambda v: None if v is None else v.detach().cpu().to(dtype)
    y = F.conv2d(t(x), t(w), None, stride, w.shape[-1] // 2)
    if scale is not None:
        y = y * t(scale)[None, :, None, None]
    if shift is not None:
        y = y + t(shift)[None, :, None, None]
    if relu:
        y = F.relu(y)
    if sigmoid_from >= 0:
        y = torch.cat((y[:, :sigmoid_from], torch.sigmoid(y[:, sigmoid_from:])), dim=1)
    if skip is not None:
        y = y + F.interpolate(t(skip), scale_factor=2, mode="nearest")
    return y.contiguous() if out_planar else y.permute(0, 2, 3, 1).contiguous()


def upsample_add64(reduced_cl, fine, dtype=torch.float64):
    """F.interpolate(reduced, size=2x, mode='bilinear') + fine at ``dtype``: reduced_cl (B,h,w,C) channel-last, fine (B,C,2h,2w)
    planar -> channel-last (B,2h,2w,C), ufr_upsample_add's layout."""
    r = reduced_cl.detach().cpu().to(dtype).permute(0, 3, 1, 2)
    up = F.interpolate(r, size=(2 * r.shape[2], 2 * r.shape[3]), mode="bilinear", align_corners=False)
    return (up + fine.detach().cpu().to(dtype)).permute(0, 2, 3, 1).contiguous()


def upsample_inputs(B: int, C: int, h: int, w: int):
    g = torch.Generator().manual_seed(100 * h + w + C)
    return torch.randn(B, h, w, C, generator=g), torch.randn(B, C, 2 * h, 2 * w, generator=g)


def upsample_add_taps(reduced_cl, fine, dtype=torch.float32, clamp_x1: bool = True):
    """The same sum tap by tap (the kernel's form: source coordinate max(0.5 (d + 0.5) - 0.5, 0), second tap clamped at the
    border).  ``clamp_x1=False``: a wrong kernel whose right-hand tap runs on into the next row at the last column."""
    r = reduced_cl.detach().cpu().to(dtype)
    B, h, w, C = r.shape
    sy = (0.5 * (torch.arange(2 * h, dtype=dtype) + 0.5) - 0.5).clamp(min=0)
    sx = (0.5 * (torch.arange(2 * w, dtype=dtype) + 0.5) - 0.5).clamp(min=0)
    y0, x0 = sy.floor().long(), sx.floor().long()
    y1 = (y0 + 1).clamp(max=h - 1)
    x1 = (x0 + 1).clamp(max=w - 1) if clamp_x1 else x0 + 1
    h1, w1 = (sy - y0).reshape(1, -1, 1, 1), (sx - x0).reshape(1, 1, -1, 1)
    flat = r.reshape(B, h * w, C)
    at = lambda yy, xx: flat[:, ((yy[:, None] * w + xx[None, :]) % (h * w)).reshape(-1)].reshape(B, 2 * h, 2 * w, C)
    up = (1 - h1) * ((1 - w1) * at(y0, x0) + w1 * at(y0, x1)) + h1 * ((1 - w1) * at(y1, x0) + w1 * at(y1, x1))
    return up + fine.detach().cpu().to(dtype).permute(0, 2, 3, 1)


def conv2d_launch(B: int, n_pixels: int):
    """launch_conv2d_t's grid, restated: (workgroups per image, groups of 256 output pixels per image).  A workgroup walks more
    than one group exactly when the first is smaller than the second."""
    n_groups = (n_pixels + 255) // 256
    blocks = min(n_groups, 1024)
    if B > 1 and blocks * B > 2048:
        blocks = (2048 + B - 1) // B
    return blocks, n_groups


# every layer shape launch_conv2d builds: (cin, cout, k, stride), and the stem (3 -> 8 from the planar image)
CONV2D_LAYERS = [(8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (32, 27, 3, 1), (32, 32, 1, 1),
                 (16, 32, 1, 1), (8, 32, 1, 1), (32, 16, 1, 1), (16, 8, 1, 1), (3, 8, 3, 1)]


def conv2d_inputs(cin, cout, k, B, H, W, seed=None):
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + k if seed is None else seed)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    return x, w, 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g), g


# ------------------------------------------------------------------ deformable convolution
def dcn_inputs(B: int, C: int, Cout: int, H: int, W: int):
    """Inputs of the deformable 3x3 layer whose taps sit ON the decisions: integer offsets that put whole rows of taps exactly
    on -1, 0, H - 1, H, W, offsets of 1e6 (far outside: the float -> int conversions), random ones elsewhere."""
    g = torch.Generator().manual_seed(7 * H + W + C)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
    bias = torch.randn(Cout, generator=g)
    off = (torch.rand(B, 18, H, W, generator=g) - 0.5) * 5.0
    mask = torch.rand(B, 9, H, W, generator=g)
    ys = torch.arange(H, dtype=torch.float32).reshape(H, 1).expand(H, W)
    xs = torch.arange(W, dtype=torch.float32).reshape(1, W).expand(H, W)
    targets_y, targets_x = [-1.0, 0.0, H - 1.0, float(H)], [-1.0, 0.0, W - 1.0, float(W)]
    for k in range(9):                               # image 0: one coordinate of every tap exactly on a target, the other free
        ki, kj = divmod(k, 3)
        if k % 2 == 0:
            off[0, 2 * k] = targets_y[(k // 2) % 4] - (ys - 1 + ki)
        else:
            off[0, 2 * k + 1] = targets_x[(k // 2) % 4] - (xs - 1 + kj)
    off[1, 0], off[1, 3], off[1, 8], off[1, 13] = 1e6, -1e6, -1e6, 1e6      # image 1: taps far outside, in y and in x, both signs
    return x, off.contiguous(), mask, w, bias
