"""Float64 yardstick of the per-ray transformers' backward that accounts for ReLU flips exactly.

A kernel's fp32 forward may put a ReLU pre-activation that lies within rounding of zero on the other side of it; the
gradient through that one unit then differs from the float64 one by an O(1) amount, not by rounding.  Instead of widening
the tolerance for that, ``envelope`` evaluates the oracle in float64 with every ReLU routed through a recorder
(``ufo_oracle._relu`` swapped), collects the AMBIGUOUS units -- ``|pre| <= tau * max|pre|`` of their call site -- and runs
one float64 backward per ambiguous unit with that unit's backward mask inverted.  ``env`` is the element-wise sum of
``|g(flip i) - g_nom|`` over them: a flip of any subset of the ambiguous units moves a gradient by at most ``env`` (the
backward is linear in each unit's mask bit).  A kernel gradient ``g`` then passes when, element-wise,

    |g - g_nom| <= eps * max(max|g_nom|, floor) + env

(``floor`` as in helpers.grad_rel_err).  ``excess`` returns the smallest ``eps`` for which that holds.

Three evaluations share the machinery: the view transformer with the radiance head (``view_envelope``: the inputs and
cotangents of ufr_view_transform_bwd), the ray transformer with DensityMLP (``ray_envelope``: ufr_ray_transform_bwd), and
both chained (``grad_envelope``: ufr_aggregate_bwd).  CPU only; the tests compare GPU gradients with the results.
"""
from __future__ import annotations

from unittest import mock

import torch

from oracle import ufo_oracle as O

TAU = 1e-5          # fp32 mode: > 10x the forward's measured 4-7e-7 relative error of a pre-activation
A_CAP = 32          # more ambiguous units than this: fail loudly (the case is too large, or tau too wide); largest seen: 26
FLOOR = 1e-5        # scale floor of helpers.grad_rel_err
# fp32 mode, of each gradient tensor's scale outside the flip envelope: the kernels' worst measured on the MI355X is 7.0e-5
# (view backward, NV 6, 4 points: linear_radianceweight_1_softmax.4.weight), 4.2e-5 (ray backward, DensityMLP.4.weight),
# 1.9e-5 (both chained), 8.2e-5 under checkpoint-like weights
EPS = 1e-4
# ... except the biases of the two MLP heads: their gradient is a plain sum over the tokens (and views) of a cotangent that
# changes sign, so it cancels, while the weight-gradient contraction rounds every term to 16 significand bits (three bf16
# plane products, wgrad_stream.hip): the error scales with sum |term| * 2^-17, the tensor with |sum term|.  Measured worst
# 1.5e-3 (view backward, NV 2, 9 points: linear_radianceweight_1_softmax.2.bias) and 2.2e-4 (DensityMLP.4.bias, whose
# true gradient is exactly the sum of d_srdf).
EPS_SUM = 6e-3
SUM_KEYS = tuple(f"ray_transformer.{m}.{i}.bias" for m in ("DensityMLP", "linear_radianceweight_1_softmax") for i in (0, 2, 4))
SHIFT_BIAS = "ray_transformer.linear_radianceweight_1_softmax.4.bias"
VIEW_TOKEN = "ray_transformer.viewToken.view_token"
VIEW_KEYS = ([O.VT + k for k in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight",
                                 "mlp.2.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
             + [f"ray_transformer.linear_radianceweight_1_softmax.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
             + [VIEW_TOKEN])
RAY_KEYS = ([O.RT + k for k in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight",
                                "mlp.2.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
            + [f"ray_transformer.DensityMLP.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")])


class _MaskedRelu(torch.autograd.Function):
    """relu whose backward mask is (pre > 0) XOR site["flip"], read when the backward runs (so one forward serves every
    flipped backward)."""

    @staticmethod
    def forward(ctx, x, site):
        ctx.site = site
        return x.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        s = ctx.site
        return g * ((s["pre"] > 0) ^ s["flip"]).to(g.dtype), None


class _Recorder:
    def __init__(self):
        self.sites = []

    def relu(self, x):
        site = dict(pre=x.detach(), flip=torch.zeros(x.shape, dtype=torch.bool))
        self.sites.append(site)
        return _MaskedRelu.apply(x, site)


class Envelope:
    """g_nom / env: {name: float64 tensor}; ambiguous: [(site, flat index, pre / max|pre| of the site)]."""

    def __init__(self, g_nom, env, ambiguous, flipped=None):
        self.g_nom, self.env, self.ambiguous, self.flipped = g_nom, env, ambiguous, flipped

    def excess(self, name, g) -> float:
        """smallest eps with |g - g_nom| <= eps * scale + env element-wise (0 when g lies inside the envelope)"""
        ref = self.g_nom[name]
        g = torch.as_tensor(g).double().cpu().reshape(ref.shape)
        scale = max(float(ref.abs().max()), FLOOR)
        return float(((g - ref).abs() - self.env[name]).clamp_min(0).max()) / scale

    def excesses(self, grads: dict) -> dict:
        """{name: excess} for every name of ``grads`` except SHIFT_BIAS (see check_shift_bias)"""
        return {k: self.excess(k, v) for k, v in grads.items() if k != SHIFT_BIAS}

    def beyond(self, grads: dict, eps: float = EPS, eps_sum: float = EPS_SUM) -> dict:
        """{name: excess} of the tensors that fail: excess > eps (eps_sum for SUM_KEYS)"""
        return {k: v for k, v in self.excesses(grads).items() if not v <= (eps_sum if k in SUM_KEYS else eps)}

    def check_shift_bias(self, g, rel: float = 1e-2) -> bool:
        """the last radiance-weight bias: its true gradient is zero (the softmax over the views is shift-invariant), so
        both sides hold rounding noise -- bounded by 1e-2 of its weight's gradient scale, as the end-to-end tests do"""
        w = self.g_nom[SHIFT_BIAS.replace("bias", "weight")]
        return float(torch.as_tensor(g).abs().max()) <= rel * float(w.abs().max())


def envelope(run, tau: float = TAU, cap: int = A_CAP, derive=None, keep_flips: bool = False) -> Envelope:
    """``run()`` -> (scalar loss, {name: tensor}) evaluated in float64; the tensors may be non-leaf.  The oracle's ReLUs
    record their pre-activations while ``run`` executes.  ``derive`` maps those gradients to the compared ones (applied to
    every flipped backward before its difference is taken).  ``keep_flips``: keep each flipped backward's gradients
    (Envelope.flipped, in the order of Envelope.ambiguous)."""
    rec = _Recorder()
    with mock.patch.object(O, "_relu", rec.relu):
        loss, wrt = run()
    names = list(wrt)
    ts = [wrt[n] for n in names]

    def grads():
        gs = torch.autograd.grad(loss, ts, retain_graph=True, allow_unused=True)
        out = {n: (torch.zeros_like(t) if g is None else g).detach() for n, g, t in zip(names, gs, ts)}
        return out if derive is None else derive(out)

    g_nom = grads()
    ambiguous = []
    for si, s in enumerate(rec.sites):
        pre = s["pre"].reshape(-1)
        top = float(pre.abs().max())
        for i in (pre.abs() <= tau * top).nonzero().reshape(-1).tolist():
            ambiguous.append((si, i, float(pre[i]) / top if top > 0 else 0.0))
    if len(ambiguous) > cap:
        raise AssertionError(f"{len(ambiguous)} ambiguous ReLU units (cap {cap}, tau {tau:g}): make the case smaller")
    env = {n: torch.zeros_like(g) for n, g in g_nom.items()}
    flipped = [] if keep_flips else None
    for si, i, _ in ambiguous:
        flip = rec.sites[si]["flip"].view(-1)
        flip[i] = True
        gf = grads()
        for n, g in gf.items():
            env[n] += (g - g_nom[n]).abs()
        flip[i] = False
        if keep_flips:
            flipped.append(gf)
    return Envelope(g_nom, env, ambiguous, flipped)


def _params(P, keys):
    return {k: (P[k].detach().double().clone().requires_grad_(k in keys)) for k in P}


def view_stage(P, x, rgbp, maskp, dirp):
    """The view-transformer half of aggregate_tokens (ray_transformer.py:284-290, 311-319): -> token0 (Pn,80), radiance (Pn,3)."""
    tok = P[VIEW_TOKEN].expand(x.shape[0], 1, 80)
    y = O.loftr_layer(torch.cat([tok, x], 1), P, O.VT)
    logit = O.mlp3(torch.cat([y[:, 1:], dirp], -1), P, "ray_transformer.linear_radianceweight_1_softmax.")
    logit = torch.where(maskp[..., None] == 0, torch.full_like(logit, -1e9), logit)
    w = torch.softmax(logit, dim=-2)
    return y[:, 0], (rgbp * w).sum(1)


def ray_stage(P, token0, RN, SN):
    """The ray-transformer half of aggregate_tokens (ray_transformer.py:292-307): token0 (RN*SN,80) -> srdf (RN,SN)."""
    pe = O.order_posenc(8, SN).to(token0)
    r = torch.cat([token0.reshape(RN, SN, 80), pe[None].expand(RN, SN, 8)], 2)
    r = O.loftr_layer(r, P, O.RT)
    return O.mlp3(r, P, "ray_transformer.DensityMLP.")[..., 0]


def _d_pv(g):
    """d x (Pn,NV,80) -> d_pv (Pn,40): the gradient of token columns 32..71 summed over the views (ufr_aggregate_bwd)"""
    g["d_pv"] = g.pop("x")[:, :, 32:72].sum(1)
    return g


def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def view_envelope(P, x, rgb, mask, dirs, d_token0, d_radiance, tau: float = TAU, cap: int = A_CAP) -> Envelope:
    """Gradients of <token0, d_token0> + <radiance, d_radiance> (either cotangent may be None = zero) w.r.t. the view
    transformer, radiance-weight MLP and view token (VIEW_KEYS) and ``d_pv`` = d x[:, :, 32:72] summed over the views."""
    def run():
        Pg = _params(P, VIEW_KEYS)
        xr = _d(x).requires_grad_(True)
        t0, rad = view_stage(Pg, xr, _d(rgb), _d(mask), _d(dirs))
        loss = sum((t * _d(c)).sum() for t, c in ((t0, d_token0), (rad, d_radiance)) if c is not None)
        return loss, dict({k: Pg[k] for k in VIEW_KEYS}, x=xr)
    return envelope(run, tau, cap, _d_pv)


def ray_envelope(P, token0, RN, SN, d_srdf, tau: float = TAU, cap: int = A_CAP) -> Envelope:
    """Gradients of <srdf, d_srdf> w.r.t. the ray transformer and DensityMLP (RAY_KEYS) and ``d_token0`` (RN*SN,80)."""
    def run():
        Pg = _params(P, RAY_KEYS)
        t0 = _d(token0).requires_grad_(True)
        loss = (ray_stage(Pg, t0, RN, SN) * _d(d_srdf).reshape(RN, SN)).sum()
        return loss, dict({k: Pg[k] for k in RAY_KEYS}, d_token0=t0)
    return envelope(run, tau, cap)


def grad_envelope(P, x, rgb, mask, dirs, RN, SN, co_rad, co_srdf, tau: float = TAU, cap: int = A_CAP,
                  keep_flips: bool = False) -> Envelope:
    """Gradients of <radiance, co_rad> + <srdf, co_srdf> through oracle.aggregate_tokens (the adjoint ufr_aggregate_bwd
    computes) w.r.t. every ray-transformer parameter it reaches (VIEW_KEYS + RAY_KEYS), ``d_pv`` and ``d_token0`` (the
    cotangent of the view transformer's token-0 output)."""
    def run():
        Pg = _params(P, VIEW_KEYS + RAY_KEYS)
        xr = _d(x).requires_grad_(True)
        want = {}
        rad, srdf = O.aggregate_tokens(Pg, xr, _d(rgb), _d(mask), _d(dirs), RN, SN, want=want)
        loss = (rad * _d(co_rad).reshape(rad.shape)).sum() + (srdf * _d(co_srdf).reshape(srdf.shape)).sum()
        return loss, dict({k: Pg[k] for k in VIEW_KEYS + RAY_KEYS}, x=xr, d_token0=want["view_out"])
    def derive(g):
        g = _d_pv(g)
        g["d_token0"] = g["d_token0"][:, 0]
        return g
    return envelope(run, tau, cap, derive, keep_flips)


def oracle_tokens(NV: int, RN: int, SN: int, seed: int = 0):
    """Token inputs of one pass through the CPU oracle on a seeded synthetic frame (for the CPU self-tests):
    x (RN*SN,NV,80), rgb (RN*SN,NV,3), mask (RN*SN,NV), dirs (RN*SN,NV,3)."""
    from uforecon_amd.scene import make_frame

    from helpers import load_weights

    P = load_weights()
    fr = make_frame(48, 64, NV, seed=40 + NV, train_layout=True)
    g = torch.Generator().manual_seed(seed)
    b = fr.batch
    idx = torch.randperm(48 * 64, generator=g)[:RN]
    ray_d = b["ray_d"][0][:, idx].t().contiguous()
    ray_o = b["ray_o"][0][None].expand(RN, 3).contiguous()
    near, far = b["near_fars"][0, 0, 0].expand(RN), b["near_fars"][0, 0, 1].expand(RN)
    pts, z = O.fixed_sample(ray_o, ray_d, near, far, torch.rand(SN, RN, generator=g))
    poses = b["source_poses"][0]
    with torch.no_grad():
        xy, _, mask_z = O.project(poses, pts)
        sim8 = O.pair_similarity(xy, fr.match_feature[0][0], NV)
        vol24 = O.volume_lookup(poses, pts, fr.feature_volume, b["near_fars"][0][0])
        x, rgb, dirs, mask = O.gather_inputs(P, pts, b, fr.source_imgs_feat[0], vol24, sim8, xy, mask_z, 1)
    Pn = RN * SN
    return (x, rgb.permute(2, 3, 0, 1).reshape(Pn, NV, 3), mask.permute(1, 2, 0).reshape(Pn, NV),
            dirs.permute(1, 2, 0, 3).reshape(Pn, NV, 3))
