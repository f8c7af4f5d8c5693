"""Every allocating wrapper once with torch's allocator and once between guard bands (tests/guarded_alloc.py).

The rest of the suite pins the kernels' VALUES; this file looks at where they touch memory.  A case of ``CASES`` builds small
inputs and calls one family of wrappers.  ``test_guard_bands`` runs it twice:

1. with the real torch (the wrapper caches cleared first), keeping the outputs;
2. with a ``GuardedTorch`` in place of ``torch`` in the wrapper modules the case goes through, the inputs copied into guarded
   buffers too (``put``).  Then: no guard byte of any output, workspace or input has changed; at least the declared number of
   allocations went through the guards (a case cannot pass because its allocations went round them); and the outputs equal
   run 1's bit for bit.  A floating ``empty`` tensor starts as NaN under the guards and as whatever the allocator held without
   them, so a result that depends on memory the kernel never wrote, or read past an input, differs.

Where a result goes through float atomics it is wrapped in ``Atomic`` with the bound the wrapper's own test uses, imported
from that test: the parameter gradients (tests/test_gpu_transformer_bwd.py: ATOMICS, with helpers.grad_rel_err), the frustum
scatter (tests/gather_ref.py: CAP_GRAD, with tests/test_gpu_gather.py's _grad_err), a whole training step's parameter
gradients (tests/test_gpu_backward.py: GRAD_TOL), the U-Nets' weight gradients (tests/unet_bwd_ref.py: ROW_BOUND with
tensor_error) and the compositor's d_variance (tests/forward_ref.py: COMPOSITE_BOUNDS).  Two host-side counts depend on how
the blocks of a launch are scheduled and are bounded, not repeated, by their own tests -- the fixpoint rounds of ``thin_points``
and the union-find rounds of ``mesh_face_components``: the masks and labels are compared bit for bit, the counts are not compared.

Shapes are the smallest at which the addressing can still go wrong: counts on both sides of a wave and a block and odd (1, 65,
257, 4097), images of 37 x 53 and 1 x 1, grids of 17 x 13 x 11, SN 16 / 48 with RN 1 / 5, NV 2 / 7, and for every count / emit
compaction an input that emits nothing, one whose every item emits and a ragged one.

``test_short_workspace_is_refused_before_anything_is_written`` takes every entry point of include/ufr.h that is given a
workspace byte count (``workspace_entry_points`` reads them from the header), runs the case that reaches it under the guards
and takes one byte off the count on its way through ctypes: the call must fail with UFR_ERR_WORKSPACE (UFR_ERR_ARG for the
four entry points whose header text says so) and the "workspace too small" text, and no byte of any guarded buffer -- guards,
outputs, workspace, inputs -- may differ from what it held just before the call.

tests/test_guarded_alloc.py (no GPU) checks that no allocating wrapper of ops.py and no such entry point is left out.
"""
from __future__ import annotations

import copy
import os
import re

import numpy as np
import pytest
import torch

import color_mesh_ref as CR
import encoder_ref as E
import forward_ref as FR
import gather_ref
import train_front_ref as TR
import unet_bwd_ref as UB
from guarded_alloc import GuardedTorch
from helpers import grad_rel_err, load_weights
from uforecon_amd import _lib, autograd, featurenet, frustum, ops, optim
from uforecon_amd.scene import fill_state_dict, make_correlate_case, make_frame, sampler_uniforms

DEV = "cuda:0"
MODULES = dict(ops=ops, autograd=autograd, frustum=frustum, featurenet=featurenet, optim=optim)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ufr.h")


# ----------------------------------------------------------------------------------------------------------- the table
class Case:
    def __init__(self, name, fn, covers, allocs, modules, refuses):
        self.name, self.fn, self.covers, self.allocs, self.modules, self.refuses = name, fn, covers, allocs, modules, refuses


CASES = {}


def case(name, covers, allocs, modules=("ops",), refuses=()):
    """``covers``: the public names of ops.py (and of the other wrapper modules, dotted) the case calls; ``allocs``: the
    outputs and workspaces those calls allocate, at least; ``refuses``: the entry points of include/ufr.h with a workspace byte
    count that the case reaches -- the refusal test shortens the first call of each"""
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = Case(name, fn, tuple(covers), int(allocs), tuple(modules), tuple(refuses))
        return fn
    return deco


class Atomic:
    """a result that goes through float atomics: ``err(got, want) < bound`` instead of equal bits"""

    def __init__(self, t, bound, err=grad_rel_err):
        self.t, self.bound, self.err = t, float(bound), err


class Put:
    """test inputs onto the device: a plain copy, or a copy between guards"""

    def __init__(self, guard=None):
        self.guard = guard

    def __call__(self, t):
        if t is None:
            return None
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if self.guard is not None:
            return self.guard.place(t.detach(), DEV)
        return t.detach().to(DEV).contiguous() if not t.is_cuda else t.detach().contiguous()

    def tree(self, x):
        if torch.is_tensor(x):
            return self(x)
        if isinstance(x, dict):
            return {k: self.tree(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(self.tree(v) for v in x)
        return x


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _rand(shape, seed, scale=1.0):
    return (torch.rand(shape, generator=_gen(seed)) - 0.5) * scale


def _cloud(n, seed, scale=1.0):
    return (torch.rand(n, 3, generator=_gen(seed), dtype=torch.float64) - 0.5) * scale


def _u8(shape, seed):
    return torch.randint(0, 256, shape, generator=_gen(seed), dtype=torch.uint8)


COUNTS = (1, 65, 257, 4097)
IMAGES = ((37, 53), (1, 1))


def clear_caches():
    """what would hand a later call an unguarded buffer of an earlier one"""
    ops._PLANES.clear()
    autograd._WS.clear()
    autograd._GWS_STATE.clear()


# ------------------------------------------------------------------------------------------------------------ ray path
def _handle(put, NV):
    fr = FR.frame(NV)
    return fr, ops.FrameHandle(put.tree(fr.batch), put(fr.source_imgs_feat), put.tree(fr.feature_volume), put.tree(fr.match_feature))


def _weights(put, precision=None):
    return ops.PackedWeights({k: put(v) for k, v in load_weights().items()}, precision=precision)


def _rays(put, NV, RN, SN, seed=0):
    ray_o, ray_d, near, far, U = FR.ray_inputs(NV, RN, SN, seed)
    return put(ray_o), put(ray_d), ops.sample_fixed(put(near), put(far), put(U))


def _gathered(put, NV, RN, SN, precision=None, **kw):
    fr, fh = _handle(put, NV)
    W = _weights(put, precision)
    o, d, z = _rays(put, NV, RN, SN)
    x, rgbm, dirs, dbg = ops.project_gather(fh, W, o, d, z, **kw)
    return fr, fh, W, o, d, z, x, rgbm, dirs, dbg


RAY_SHAPES = ((2, 5, 16), (7, 1, 48))       # (NV, RN, SN)


@case("sample_fixed", ["sample_fixed"], allocs=4)
def _sample_fixed(put):
    out = []
    for RN, SN in ((1, 16), (5, 48), (65, 16), (257, 48)):
        g = _gen(RN)
        near = 1.5 + torch.rand(RN, generator=g)
        out.append(ops.sample_fixed(put(near), put(near + 1.0 + torch.rand(RN, generator=g)), put(torch.rand(SN, RN, generator=g))))
    return out


@case("sample_importance", ["sample_importance_merge", "sample_importance_pool"], allocs=3 * 5 + 1)
def _sample_importance(put):
    out = []
    for SN, PN in ((16, 16), (17, 5), (48, 16)):
        w, z, U2 = (put(t) for t in FR.sampler_inputs(SN, PN))
        out.append(ops.sample_importance_merge(w, z, U2))
        out.append(ops.sample_importance_pool(w, z, U2))
    w, z, U2 = (put(t) for t in FR.sampler_inputs(3, 7, "zero_run"))
    out.append(ops.sample_importance_merge(w, z, U2, want_fine=False))
    return out


@case("points", ["points"], allocs=3)
def _points(put):
    out = []
    for RN, SN, per_ray in ((1, 16, False), (5, 48, True), (257, 3, True)):
        o = _rand((RN, 3) if per_ray else (3,), RN)
        out.append(ops.points(put(o), put(_rand((RN, 3), RN + 1)), put(2.0 + torch.rand(RN, SN, generator=_gen(RN + 2)))))
    return out


@case("project_gather", ["FrameHandle", "PackedWeights", "project_gather"], allocs=2 * (2 + 3 + 4) + 2,
      refuses=["ufr_frame_prepare"])
def _project_gather(put):
    out = []
    for NV, RN, SN in RAY_SHAPES:
        fr, fh, W, o, d, z, x, rgbm, dirs, dbg = _gathered(put, NV, RN, SN, debug=True)
        out.append((x, rgbm, dirs, dbg))
        out.append(ops.project_gather(fh, W, o, d, z, want_sim8=True, want_xy=True))
        assert ops.status_poll(True) == 0
    return out


@case("aggregate", ["aggregate", "view_transform", "ray_transform"], allocs=2 * (5 + 3 + 2 + 2))
def _aggregate(put):
    out = []
    for (NV, RN, SN), prec in zip(RAY_SHAPES, (ops.PRECISION_FP32, ops.PRECISION_16BIT)):
        fr, fh, W, o, d, z, x, rgbm, dirs, _ = _gathered(put, NV, RN, SN)
        out.append(ops.aggregate(W, x, rgbm, dirs, RN, SN, debug=True, keep_workspace=True, precision=prec))
        out.append(ops.aggregate(W, x, rgbm, dirs, RN, SN, precision=1 - prec))
        token0, radiance = ops.view_transform(W, x, rgbm, dirs, precision=prec)
        out.append((token0, radiance, ops.ray_transform(W, token0, RN, SN, precision=prec)))
        assert ops.status_poll(True) == 0
    return out


@case("composite", ["composite", "composite_bwd"], allocs=3 * (4 + 3))
def _composite(put):
    out = []
    for SN, RN in ((17, 5), (65, 1), (200, 65)):
        c = {k: put(v) for k, v in FR.composite_inputs(SN, RN).items()}
        var = put(torch.tensor(0.3))
        out.append(ops.composite(c["z"], c["radiance"], c["srdf"], var))
        d_radiance, d_srdf, d_var = ops.composite_bwd(c["z"], c["radiance"], c["srdf"], var, c["d_rgb"], c["d_depth"], c["d_opacity"],
                                                      c["d_weight"])
        # every ray adds its share to d_variance with one float atomic (csrc/composite.hip): the order is not fixed.  (At 65 rays
        # the shares cancel to a sixth of their magnitudes' sum: no order of 65 float adds moves the sum by more than 65 x 2^-24 x 6
        # = 2.3e-5 of itself, inside the bound.)
        out.append((d_radiance, d_srdf, Atomic(d_var, FR.COMPOSITE_BOUNDS["d_variance"], _rel_scalar)))
    return out


@case("render_loss", ["render_loss"], allocs=3)
def _render_loss(put):
    out = []
    for B, RN in ((1, 1), (1, 65), (2, 257)):
        g = _gen(B * 1000 + RN)
        r = lambda *s: torch.rand(*s, generator=g)
        depth_gt = 2.0 + r(B, RN)
        depth_gt[:, ::3] = 0.0          # outside the near / far range: no depth term
        nf = torch.tensor([1.5, 3.5]).expand(B, 4, 2).contiguous()
        out.append(ops.render_loss(put(r(B, RN, 3)), put(2.0 + r(B, RN)), put(r(B, RN, 3)), put(2.0 + r(B, RN)), put(r(B, RN, 3)),
                                   put(depth_gt), put(nf), 1.0, 0.5))
    return out


def _rel_scalar(got, want):
    """FR.composite_errors' form for d_variance: relative to the value itself"""
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-30)


def _param_grads(grads):
    return {k: Atomic(v, ATOMICS()) for k, v in grads.views.items()}


def ATOMICS():
    import test_gpu_transformer_bwd

    return test_gpu_transformer_bwd.ATOMICS


@case("aggregate_bwd", ["GradBuffer", "aggregate_bwd"], allocs=2 * (1 + 2))
def _aggregate_bwd(put):
    out = []
    for (NV, RN, SN), prec in zip(RAY_SHAPES, (ops.PRECISION_FP32, ops.PRECISION_16BIT)):
        fr, fh, W, o, d, z, x, rgbm, dirs, _ = _gathered(put, NV, RN, SN)
        _, _, dbg = ops.aggregate(W, x, rgbm, dirs, RN, SN, keep_workspace=True, precision=prec)
        grads = ops.GradBuffer(DEV)
        d_pv, _ = ops.aggregate_bwd(W, grads, x, rgbm, dirs, dbg["token0"], RN, SN, put(_rand((RN * SN, 3), 5)), put(_rand((RN, SN), 6)),
                                    precision=prec)
        assert ops.status_poll(True) == 0
        out.append((d_pv, _param_grads(grads)))
    return out


@case("project_gather_bwd", ["project_gather_bwd", "project_gather_bwd_workspace_floats"], allocs=2 * 2)
def _project_gather_bwd(put):
    import test_gpu_gather

    out = []
    for NV, RN, SN in RAY_SHAPES:
        fr, fh, W, o, d, z, x, rgbm, dirs, dbg = _gathered(put, NV, RN, SN, want_sim8=True)
        grads = ops.GradBuffer(DEV)
        shapes = [tuple(fr.feature_volume[st][k].shape) for st in gather_ref.STAGES for k in ("feature_volume", "weight_volume")]
        targets = [put(torch.full(s, 7.0)) for s in shapes]
        ops.project_gather_bwd(fh, W, grads, o, d, z, dbg["sim8"], put(_rand((RN * SN, 40), NV)), targets[0::2], targets[1::2],
                               accumulate=False)
        assert ops.status_poll(True) == 0
        out.append(([Atomic(t, gather_ref.CAP_GRAD, test_gpu_gather._grad_err) for t in targets], _param_grads(grads)))
    return out


@case("transformer_tape_and_backward",
      ["view_transform_tape", "ray_transform_tape", "ray_transform_bwd", "ray_transform_bwd_workspace", "view_transform_bwd",
       "view_transform_bwd_workspace"], allocs=2 * (2 + 1 + 2 + 1 + 3 + 1))
def _tape(put):
    out = []
    for (NV, RN, SN), prec in zip(RAY_SHAPES, (ops.PRECISION_FP32, ops.PRECISION_16BIT)):
        fr, fh, W, o, d, z, x, rgbm, dirs, _ = _gathered(put, NV, RN, SN)
        P = RN * SN
        d_rad, d_srdf = put(_rand((P, 3), 11)), put(_rand((RN, SN), 12))
        # the tape recorded by the forward, the backward from the data gradients on
        grads = ops.GradBuffer(DEV)
        vws, rws = ops.view_transform_bwd_workspace(P, NV, DEV), ops.ray_transform_bwd_workspace(RN, SN, DEV)
        token0, radiance = put(torch.full((P, 80), float("nan"))), put(torch.full((P, 3), float("nan")))
        ops.view_transform_tape(W, x, rgbm, dirs, token0, radiance, vws, 0, P, precision=prec)
        srdf = ops.ray_transform_tape(W, token0, RN, SN, rws, precision=prec)
        rest = ops.STAGE_DGRAD | ops.STAGE_WGRAD
        a, b = ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, precision=prec, stages=rest, workspace=rws)
        d_pv = ops.view_transform_bwd(W, grads, x, rgbm, dirs, a, b, d_rad, precision=prec, stages=rest, workspace=vws)
        assert ops.status_poll(True) == 0
        out.append((token0, radiance, srdf, a, b, d_pv, _param_grads(grads)))
        # the backward that builds its own tape and allocates its own workspaces
        grads = ops.GradBuffer(DEV)
        a, b = ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, precision=prec)
        d_pv = ops.view_transform_bwd(W, grads, x, rgbm, dirs, a, b, d_rad, precision=prec)
        assert ops.status_poll(True) == 0
        out.append((a, b, d_pv, _param_grads(grads)))
    return out


def _render(put, NV, RN, SN, PN, prec, chunk, lanes=2, **kw):
    fr, fh = _handle(put, NV)
    W = _weights(put, prec)
    idx = torch.randperm(48 * 64, generator=_gen(RN))[:RN]
    U1, U2 = sampler_uniforms(NV, SN, max(PN, 1), RN)
    ws = ops.RenderWorkspace(DEV, SN, PN, NV, chunk_rays=chunk, n_streams=lanes)
    out = ops.render_rays(fh, W, put(idx), put(U1), put(U2) if PN else None, workspace=ws, **kw)
    assert ops.status_poll(True) == 0
    return {k: v for k, v in out.items() if k != "workspace"}


@case("render_rays", ["RenderWorkspace", "render_rays"], allocs=2 * (2 + 6) + 2 + 4, refuses=["ufr_render_rays"])
def _render_rays(put):
    # 37 rays in chunks of 16.  One lane first: with more, a workspace that is short of them renders on fewer lanes (csrc/api_ray.hip),
    # and the refusal test wants the call that is refused
    return [_render(put, 2, 37, 16, 16, ops.PRECISION_FP32, 16, lanes=1),
            _render(put, 7, 5, 48, 16, ops.PRECISION_16BIT, 16),
            _render(put, 2, 1, 16, 0, ops.PRECISION_FP32, 16, coarse_only=True)]


@case("render_rays_pair", ["RenderWorkspace", "render_rays"], allocs=2 * (2 + 8), refuses=["ufr_render_rays_pair"])
def _render_pair(put):
    return [_render(put, 2, 37, 16, 16, ops.PRECISION_16BIT, 16, lanes=1, pair=True),
            _render(put, 7, 5, 48, 16, ops.PRECISION_FP32, 16, pair=True)]


@case("frame_metrics", ["frame_metrics", "frame_preview_u8"], allocs=2 * 4)
def _frame_metrics(put):
    out = []
    for H, W in IMAGES:
        n = H * W
        g = _gen(n)
        r = lambda *s: torch.rand(*s, generator=g)
        depth_gt = 2.0 + r(n)
        depth_gt[::5] = 0.0
        m = ops.frame_metrics(put(r(n, 3)), put(r(n, 3)), put(r(3, n)), put(2.0 + r(n)), put(2.0 + r(n)), put(depth_gt), 1.5, 3.5)
        out.append(m)
        out.append(ops.frame_preview_u8(put(r(n, 3)), put(2.0 + r(n)), m[7:8].clone(), 0.5))
    return out


@case("fmt_layer", ["fmt_layer"], allocs=3 * 2)
def _fmt_layer(put):
    from uforecon_amd import fmt

    p = copy.deepcopy(E.fmt_params()).to(DEV)
    out = []
    with torch.no_grad():
        for c, mode in ((E.FMT_CASES[0], "self"), (E.FMT_CASES[1], "cross"), (E.FMT_CASES[1], "self_long")):
            x, src = E.fmt_tokens(*c, mode)
            out.append(fmt._layer(p, put(x), put(src)))
    return out


# ------------------------------------------------------------------------------------------------------------ encoder
@case("conv2d", ["conv2d", "upsample_add", "deform_conv2d_cl"], allocs=6 + 2 + 2)
def _conv2d(put):
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()
    out = []
    x, w, sc, sh, _ = E.conv2d_inputs(8, 8, 3, 2, 37, 53)
    out.append(ops.conv2d(put(cl(x)), put(w), 1, put(sc), put(sh), relu=True))
    x, w, sc, sh, _ = E.conv2d_inputs(8, 8, 3, 1, 1, 1)
    out.append(ops.conv2d(put(cl(x)), put(w), 1, put(sc), put(sh), relu=True))
    x, w, sc, sh, _ = E.conv2d_inputs(8, 16, 5, 1, 37, 53)
    out.append(ops.conv2d(put(cl(x)), put(w), 2, put(sc), put(sh), relu=True, out_planar=True))
    x, w, sc, sh, _ = E.conv2d_inputs(3, 8, 3, 2, 37, 53)
    out.append(ops.conv2d(put(x), put(w), 1, put(sc), put(sh), relu=True, in_planar=True))
    x, w, sc, sh, _ = E.conv2d_inputs(32, 27, 3, 1, 9, 13)
    out.append(ops.conv2d(put(cl(x)), put(w), 1, None, put(sh), out_planar=True, sigmoid_from=18))
    x, w, sc, sh, g = E.conv2d_inputs(16, 32, 1, 1, 18, 26)
    out.append(ops.conv2d(put(cl(x)), put(w), 1, None, put(sh), skip=put(torch.randn(1, 9, 13, 32, generator=g))))
    for B, C, h, w_ in ((1, 16, 9, 13), (2, 8, 1, 1)):            # the kernel is built for C of 8 and 16
        r, fine = E.upsample_inputs(B, C, h, w_)
        out.append(ops.upsample_add(put(r), put(fine)))
    x, off, mask, w, bias = E.dcn_inputs(2, 32, 32, 9, 13)
    x_cl, om = put(cl(x)), put(torch.cat([off, mask], 1))
    out.append(ops.deform_conv2d_cl(x_cl, om, put(w), put(bias)))
    out.append(ops.deform_conv2d_cl(x_cl, om, put(w), put(bias), put(0.5 + torch.rand(32, generator=_gen(1))), put(_rand((32,), 2)),
                                    relu=True, out_planar=True))
    return out


@case("featurenet", ["conv2d", "deform_conv2d_cl", "featurenet.feature_net", "featurenet.deform_conv2d"], allocs=31 + 2,
      modules=("ops", "featurenet"), refuses=["ufr_deform_conv2d"])
def _featurenet(put):
    x, off, mask, w, bias = E.dcn_inputs(2, 32, 32, 9, 13)
    out = [featurenet.deform_conv2d(put(x), put(off), put(w), put(bias), 1, 1, 1, mask=put(mask))]
    net = fill_state_dict(featurenet.FeatureNet(), 5).eval().to(DEV)
    with torch.no_grad():
        out.append(net(put(torch.rand(1, 3, 36, 52, generator=_gen(3)))))
    return out


def _correlate_calls(put, c):
    args = (put(c["ref_fea"]), put(torch.stack(c["src_feas"])), c["ref_proj_pair"], c["src_proj_pairs"], put(c["depth_values"]))
    vw = put(c["view_weights"])
    return [frustum.correlate(*args, vw), frustum.correlate(*args, None), frustum.correlate(*args, vw, want_similarity=False)]


@case("frustum_correlate", ["frustum.correlate", "frustum.view_weights"], allocs=2 * 7 + 2, modules=("ops", "frustum"),
      refuses=["ufr_frustum_correlate"])
def _correlate(put):
    from uforecon_amd import cascade

    out = []
    for over in (dict(C=4, H=9, W=13, D=9, NV=2, seed=61), dict(C=64, H=8, W=10, D=5, NV=4, seed=65)):     # every LP: C of 4 and 64
        out.append(_correlate_calls(put, make_correlate_case("custom", **over)))
    net = fill_state_dict(cascade.PixelwiseNet(), 4).eval().to(DEV)
    with torch.no_grad():
        out.append(frustum.view_weights(net, put(E.pixelwise_sim(3, 8, 17, 23, 1.0))))
    return out


# ------------------------------------------------------------------------------------------------------------- U-Nets
GRID = (1, 11, 13, 17)      # (B, D, H, W): no extent a multiple of 4


def _x3d(put, c, seed, dims=GRID):
    return put(torch.randn(*dims, c, generator=_gen(seed)))


def _w3d(put, shape, seed):
    return put(torch.randn(*shape, 3, 3, 3, generator=_gen(seed)) * 0.2)


@case("conv3d", ["conv3d", "absmax"], allocs=1 + 1 + 1 + 2 + 2 + 3)
def _conv3d(put):
    B, D, H, W = GRID
    out = []
    x8, x16 = _x3d(put, 8, 1), _x3d(put, 16, 2)
    out.append(ops.conv3d(x8, _w3d(put, (8, 8), 3), ops.CONV3D_S1, bias=put(_rand((8,), 4)), relu=True,
                          skip=put(_rand((B, D, H, W, 8), 5))))
    out.append(ops.conv3d(x8, _w3d(put, (16, 8), 6), ops.CONV3D_S2, bn_scale=put(0.5 + torch.rand(16, generator=_gen(7))),
                          bn_shift=put(_rand((16,), 8)), relu=True))
    out.append(ops.conv3d(x16, _w3d(put, (16, 8), 9), ops.CONV3D_T2))
    out.append(ops.conv3d(x8, _w3d(put, (8, 8), 10), ops.CONV3D_S1, out_ncdhw=True, weight2=_w3d(put, (1, 8), 11)))
    out.append(ops.conv3d(x8, _w3d(put, (8, 8), 12), ops.CONV3D_S1, want_absmax=True))
    for n in (1, 65, 4097):
        out.append(ops.absmax(put(_rand((n,), n, 9.0))))
    return out


@case("conv3d_planes", ["conv3d_planes", "absmax"], allocs=4 * 7 + 3 * 4 + 3 * 4 + 4, refuses=["ufr_conv3d_planes"])
def _conv3d_planes(put):
    out = []
    dims = (1, 3, 9, 37)
    for cin in (8, 16, 32, 64):
        x = _x3d(put, cin, cin, dims)
        am = ops.absmax(x)
        for flip in (False, True):
            out.append(ops.conv3d_planes(x, am, _w3d(put, (cin, cin), cin + flip), bias=None if flip else put(_rand((cin,), 1)),
                                         skip=put(_rand((*dims, cin), 2)), flip=flip))
    for cin in (8, 16, 32):
        x = _x3d(put, cin, 100 + cin, dims)
        out.append(ops.conv3d_planes(x, ops.absmax(x), _w3d(put, (2 * cin, cin), cin), bias=put(_rand((2 * cin,), 3)), relu=True,
                                     mode=ops.CONV3D_S2))
    for cin in (16, 32, 64):
        x = _x3d(put, cin, 200 + cin, (1, 3, 5, 18))
        out.append(ops.conv3d_planes(x, ops.absmax(x), _w3d(put, (cin, cin // 2), cin), bias=put(_rand((cin // 2,), 4)),
                                     mode=ops.CONV3D_T2))
    x = _x3d(put, 8, 300, dims)
    out.append(ops.conv3d_planes(x, ops.absmax(x), _w3d(put, (8, 8), 5), out_ncdhw=True, weight2=_w3d(put, (1, 8), 6)))
    return out


@case("conv3d_bwd", ["conv3d_bwd_data", "conv3d_bwd_weight", "conv3d_bwd_weight_heads"], allocs=3 + 3 * 2 + 2)
def _conv3d_bwd(put):
    B, D, H, W = GRID
    # the weight-gradient kernels add their bricks' partial sums with float atomics (csrc/conv3d.hip, conv3d_wgrad_planes.hip)
    wgrad = lambda ts: [Atomic(t, UB.ROW_BOUND, UB.tensor_error) for t in ts]
    even = (B, 10, 14, 18)                      # the strided layer's data gradient takes even extents only
    out = []
    # (mode, cin, cout, extent of the layer's input, extent of d_out, weight shape)
    for mode, cin, cout, xd, od, wshape in ((ops.CONV3D_S1, 8, 8, GRID, GRID, (8, 8)), (ops.CONV3D_S2, 8, 16, even, (B, 5, 7, 9), (16, 8)),
                                            (ops.CONV3D_T2, 16, 8, GRID, (B, 2 * D, 2 * H, 2 * W), (16, 8))):
        x, d_out, w = _x3d(put, cin, mode, xd), _x3d(put, cout, 10 + mode, od), _w3d(put, wshape, 20 + mode)
        out.append(ops.conv3d_bwd_data(d_out, w, mode, (*xd, cin), accumulate=put(_rand((*xd, cin), 30 + mode))))
        out.append(wgrad(ops.conv3d_bwd_weight(x, d_out, mode, (*wshape, 3, 3, 3))))
    out.append(wgrad(ops.conv3d_bwd_weight_heads(_x3d(put, 8, 40), _x3d(put, 8, 41), _x3d(put, 1, 42))))
    return out


# ----------------------------------------------------------------------------------------------------------- geometry
def _volumes():
    X, Y, Z = 17, 13, 11
    i, j, k = torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij")
    sphere = ((i - 8.2) ** 2 + (j - 6.1) ** 2 + (k - 5.3) ** 2).float().sqrt() - 4.4
    return dict(nothing=torch.ones(X, Y, Z), every_cell=(((i + j + k) % 2) * 2 - 1).float() * 0.5, ragged=sphere, smallest=sphere[:2, :2, :2] + 4.0)


@case("marching_cubes", ["marching_cubes"], allocs=4 * 4, refuses=["ufr_marching_cubes_count", "ufr_marching_cubes_emit"])
def _marching_cubes(put):
    v = _volumes()
    return [ops.marching_cubes(put(v[k].contiguous())) for k in ("ragged", "nothing", "every_cell", "smallest")]


@case("similarity_field", ["similarity_field"], allocs=2 * 2)
def _similarity_field(put):
    out = []
    for NV in (2, 7):
        _, fh = _handle(put, NV)
        out.append(ops.similarity_field(fh, [-0.9] * 3, [0.8] * 3, (17, 13, 11), min_views=2, return_visibility=True))
        assert ops.status_poll(True) == 0
    return out


def _mesh(level, stretch=(1.0, 1.0, 1.0)):
    v, f = CR.icosphere(level)
    return torch.from_numpy(v * np.asarray(stretch)), torch.from_numpy(f)


@case("chamfer", ["cell_keys", "sample_mesh", "thin_points", "nn_distance"], allocs=3 * 2 + 4 * (1 + 4 + 6),
      refuses=["ufr_mesh_sample_count", "ufr_mesh_sample_emit", "ufr_points_thin", "ufr_points_nn_dist"])
def _chamfer(put):
    out = []
    # ragged (stretched triangles of several sizes), nothing sampled (a density coarser than every edge), every face sampled
    for level, stretch, density in ((2, (3.0, 1.0, 0.3), 0.2), (1, (1.0, 1.0, 1.0), 50.0), (1, (1.0, 1.0, 1.0), 0.05)):
        v, f = _mesh(level, stretch)
        out.append(ops.sample_mesh(put(v), put(f), density))
    for n in COUNTS:
        p = put(_cloud(n, n))
        out.append(ops.cell_keys(p, (-1.0, -1.0, -1.0), 0.07))
        # the keep-mask is the sequential loop's, whatever the scheduling; the NUMBER of fixpoint rounds is not (a round reads the
        # states other blocks are writing, csrc/chamfer.hip), and tests/test_chamfer.py only bounds it: not compared
        keep, rounds = ops.thin_points(p, 0.08, return_rounds=True)
        assert rounds >= 1
        out.append(keep)
        out.append(ops.nn_distance(p, put(_cloud(max(1, n // 2), n + 1)), 0.2, return_sums=True))
    return out


@case("pcd_filter", ["knn_points", "point_normals", "voxel_downsample"], allocs=4 * (3 * 6 + 5 + 6 + 3),
      refuses=["ufr_points_voxel_mean"])
def _pcd_filter(put):
    out = []
    for n in COUNTS:
        p = put(_cloud(n, 10 + n))
        # ragged voxels; every point its own voxel; all points in one voxel
        for voxel in (0.11, 1e-4, 4.0):
            out.append(ops.voxel_downsample(p, voxel, colors=put(_u8((n, 3), n)), normals=put(_cloud(n, 20 + n))))
        k = min(7, n)
        idx, dist = ops.knn_points(p, p, k, exclude_self=False)
        out.append((idx, dist))
        out.append(ops.knn_points(put(_cloud(65, 30 + n)), p, min(32, n), max_dist=0.3))
        out.append(ops.point_normals(p, idx, viewpoints=put(_cloud(2, 40 + n, 6.0))))
    return out


@case("poisson", ["poisson_splat", "poisson_divergence", "poisson_laplacian", "poisson_solve", "poisson_sample"],
      allocs=2 * (3 + 1 + 1 + 2 + 3), refuses=["ufr_poisson_solve", "ufr_poisson_sample"])
def _poisson(put):
    out = []
    for n, res in ((257, 9), (4097, 14)):
        c = _cloud(n, 50 + n)
        nrm = c / c.norm(dim=1, keepdim=True)
        p, nr = put(nrm * 0.7 + 0.1), put(nrm)
        origin, h, dims = ops.poisson_grid(p, resolution=res, pad=2)
        V, Wt = ops.poisson_splat(p, nr, origin, h, dims)
        b = ops.poisson_divergence(V, h)
        x, info = ops.poisson_solve(b, h, max_iter=24, check_every=8)
        out.append((V, Wt, b, ops.poisson_laplacian(b, h), x, info["iterations"], info["residual"],
                    ops.poisson_sample(x, origin, h, p, return_mean=True)))
    return out


def _camera(H, W, eye=(0.3, -3.0, 0.4)):
    """(K 3x3, c2w 4x4, E = w2c 4x4) float64 of a camera that looks at the origin"""
    K = CR.intrinsics(H, W, 0.9 * max(W, 2))
    c2w = CR.look_at(eye)
    return K, c2w, np.linalg.inv(c2w)


@case("depth_fusion", ["depth_consistency", "depth_points"], allocs=2 * 4 + 6 * 3,
      refuses=["ufr_depth_points_count", "ufr_depth_points_emit"])
def _depth_fusion(put):
    from uforecon_amd import depth_fusion as DF

    out = []
    for H, W in IMAGES:
        K, c2w, Eref = _camera(H, W)
        srcs = [np.linalg.inv(CR.look_at(e)) for e in ((0.5, -3.0, 0.4), (0.1, -3.0, 0.6))]
        mats = np.stack([DF.pair_matrices(K, Eref, K, Es) for Es in srcs])
        g = _gen(H)
        depth = lambda h, w: put(2.8 + 0.4 * torch.rand(h, w, generator=g))
        out.append(ops.depth_consistency(depth(H, W), [depth(H, W), depth(H + 3, W + 2)], put(mats), return_pair_masks=True))
        avg, color = put(2.8 + 0.4 * torch.rand(H, W, generator=g, dtype=torch.float64)), put(_u8((H, W, 3), H))
        ragged = (torch.rand(H, W, generator=g) < 0.4).to(torch.uint8) * 255
        for mask in (ragged, torch.zeros(H, W, dtype=torch.uint8), torch.full((H, W), 255, dtype=torch.uint8)):
            out.append(ops.depth_points(put(mask), avg, color, np.linalg.inv(K), c2w))
    return out


@case("mesh_clean", ["dilate_mask", "mesh_vertex_votes", "mesh_first_hit", "mesh_face_components"], allocs=2 * 2 + 1 + 2 * 3 + 2 * 3,
      refuses=["ufr_mesh_first_hit", "ufr_mesh_face_components"])
def _mesh_clean(put):
    from uforecon_amd import clean_mesh as CM

    out = []
    for H, W in IMAGES:
        img = _u8((H, W), H)
        out.append(ops.dilate_mask(put(img), 11, return_dilated=True))
    H, W = IMAGES[0]
    K, _, Ew = _camera(H, W)
    v, f = _mesh(2)
    f = torch.cat([f, f[:3]])           # duplicate faces: edges that more than two faces share
    masks = (torch.rand(2, H, W, generator=_gen(9)) < 0.7).to(torch.uint8)
    P = np.stack([(K @ Ew[:3]), (K @ np.linalg.inv(CR.look_at((-0.4, -3.0, 0.1)))[:3])]).astype(np.float32)
    out.append(ops.mesh_vertex_votes(put(v), put(P), put(masks)))
    for (h, w), vv, ff in ((IMAGES[0], v, f), (IMAGES[1], *_mesh(0))):
        Kc, _, Ec = _camera(h, w)
        k_inv, c2w32 = CM.ray_camera(Kc, Ec)
        out.append(ops.mesh_first_hit(put(vv), put(ff), k_inv, c2w32, put(torch.ones(h, w, dtype=torch.uint8))))
        # the labels are fixed; how many union-find rounds pass until nothing changes depends on how the hooks and jumps of one
        # launch interleave (csrc/mesh_clean.hip), and tests/test_clean_mesh.py only bounds it: not compared
        labels, rounds = ops.mesh_face_components(put(vv), put(ff), return_rounds=True)
        assert rounds >= 1
        out.append(labels)
    return out


@case("raster", ["raster_vertex_normals", "raster_frames", "raster_downsample", "splat_frames"], allocs=1 + 2 * 4 + 3 + 2 * 3,
      refuses=["ufr_raster_frames", "ufr_splat_frames"])
def _raster(put):
    out = []
    v, f = _mesh(2)
    tv, tf = put(v), put(f)
    normals = ops.raster_vertex_normals(tv, tf)
    out.append(normals)
    colors = put(_u8((v.shape[0], 3), 3))
    for H, W in IMAGES:
        K, c2w, Ew = _camera(H, W)
        c2ws = np.stack([c2w, CR.look_at((2.0, -2.0, 1.0))])
        out.append(ops.raster_frames(tv, tf, np.linalg.inv(K / K[2, 2]), c2ws, H, W, normals=normals, colors=colors, return_depth=True,
                                     return_face_ids=True, return_normals=True))
        pts = put(_cloud(4097 if H > 1 else 1, H, 1.6))
        out.append(ops.splat_frames(pts, K / K[2, 2], np.linalg.inv(c2ws), H, W, colors=put(_u8((pts.shape[0], 3), 4)), radius=2,
                                    edl_strength=0.7, edl_radius=2, return_depth=True, return_point_ids=True))
    for s, (H, W) in ((3, (3 * 37, 3 * 53)), (2, (2 * 37, 2 * 53)), (4, (4, 4))):          # supersampled frames and their downsample
        K, c2w, _ = _camera(H, W)
        big = ops.raster_frames(tv, tf, np.linalg.inv(K / K[2, 2]), c2w[None], H, W)["image"]
        out.append(ops.raster_downsample(put(big), s))
    return out


@case("mesh_color", ["mesh_vertex_colors", "mesh_color_fill"], allocs=2 * 3 + 2 * 3, refuses=["ufr_color_vertices"])
def _mesh_color(put):
    out = []
    H, W = IMAGES[0]
    for level in (0, 3):
        v, f = _mesh(level)
        tv, tf = put(v), put(f)
        normals = put(v / v.norm(dim=1, keepdim=True))
        c2ws = [CR.look_at((0.3, -3.0, 0.4)), CR.look_at((2.0, 2.0, -1.0)), CR.look_at((-3.0, 0.2, 0.1))]
        K = CR.intrinsics(H, W, 0.9 * W)
        cams = [CR.projection_camera(K, c) for c in c2ws]
        k, w2c, centre = (np.stack([c[i] for c in cams]) for i in range(3))
        depth = torch.stack([ops.raster_frames(tv, tf, np.linalg.inv(K / K[2, 2]), c[None].astype(np.float32), H, W,
                                               return_depth=True)["depth"][0] for c in c2ws])
        imgs = put(_u8((3, H, W, 3), level))
        for mode, dep in (("mean", put(depth)), ("best", None)):
            col, used = ops.mesh_vertex_colors(tv, normals, imgs, dep, k, w2c, centre, mode=mode)
            out.append((col, used, ops.mesh_color_fill(tf, col, used, 3)))
    return out


def _simplify_chain(put, v, f, cell, colors):
    """mesh_simplify's steps one by one, every intermediate result between guards before the next step reads it"""
    verts, faces, cols = put(v), put(f), put(colors)
    mn = verts.min(0).values
    origin = (mn - cell / 2).tolist()
    keys, order = (put(t) for t in torch.sort(ops.cell_keys(verts, origin, cell), stable=True))
    cluster, ckey = ops.simplify_clusters(keys, order)
    mean, ccol, _, count = ops.voxel_downsample(verts, cell, colors=cols)
    fkeys = put(torch.sort(ops.simplify_face_keys(faces, cluster), stable=True).values)
    quadrics, n_faces = ops.simplify_quadrics(verts, faces, put(ckey), origin, cell, fkeys)
    position, placed = ops.simplify_place(quadrics, n_faces, put(mean), put(ckey), origin, cell)
    triples, key_a, key_bc = ops.simplify_face_triples(faces, cluster)
    keep = ops.simplify_face_heads(key_a, key_bc)
    out_faces, face_map, referenced = ops.simplify_compact_faces(triples, keep, int(ckey.shape[0]))
    out_faces = put(out_faces)
    compact = ops.simplify_compact_vertices(referenced, position, put(ccol), placed, put(count), cluster, out_faces)
    return (cluster, ckey, mean, ccol, count, quadrics, n_faces, position, placed, triples, key_a, key_bc, keep, out_faces, face_map,
            referenced, compact)


@case("mesh_simplify",
      ["simplify_clusters", "simplify_face_keys", "simplify_quadrics", "simplify_place", "simplify_face_triples", "simplify_face_heads",
       "simplify_compact_faces", "simplify_compact_vertices", "simplify_count_cells", "simplify_target_cell", "mesh_simplify",
       "cell_keys", "voxel_downsample"], allocs=3 * 29 + 2 * 25 + 2,
      refuses=["ufr_simplify_clusters", "ufr_simplify_compact_faces", "ufr_simplify_compact_vertices"])
def _mesh_simplify(put):
    out = []
    v, f = _mesh(2, (1.0, 0.8, 0.6))
    colors = _u8((v.shape[0], 3), 7)
    # ragged clusters; every vertex its own cluster (every item emits); one cluster (every face collapses: nothing to emit)
    for cell in (0.45, 1e-3, 8.0):
        out.append(_simplify_chain(put, v, f, cell, colors))
    tv, tf = put(v), put(f)
    out.append(ops.simplify_count_cells(tv, 0.45))
    r = ops.mesh_simplify(tv, tf, colors=put(colors), cell=0.45)
    out.append(r)
    out.append(ops.mesh_simplify(tv, tf, target_vertices=65, placement="mean"))
    v1, f1 = _mesh(0)
    out.append(ops.mesh_simplify(put(v1), put(f1), cell=8.0))
    return out


@case("mesh_smooth", ["mesh_smooth", "mesh_denoise"], allocs=3 * 3 + 2 * 4,
      refuses=["ufr_smooth_rows", "ufr_smooth_steps", "ufr_denoise_faces", "ufr_denoise_normals", "ufr_denoise_vertices"])
def _mesh_smooth(put):
    out = []
    for level in (0, 3):
        v, f = _mesh(level)
        f = f[: f.shape[0] - 3]                    # a hole: border vertices
        v = v + _cloud(v.shape[0], level, 0.02)
        tv, tf = put(v), put(f)
        pinned = put((torch.arange(v.shape[0]) % 7 == 0).to(torch.uint8))
        out.append(ops.mesh_smooth(tv, tf, "taubin", "cotangent", iterations=3, pinned=pinned))
        out.append(ops.mesh_smooth(tv, tf, "laplacian", "uniform", iterations=3, boundary="free"))
        out.append(ops.mesh_denoise(tv, tf, normal_iterations=2, vertex_iterations=3, sigma_s=0.3, pinned=pinned))
    return out


# -------------------------------------------------------------------------------------------------------------- loaders
@case("image_loaders", ["image_resize_u8", "image_resize_mask_u8", "image_undistort_u8", "pixel_rays", "depth_gt_prepare"],
      allocs=2 + 2 + 4 + 2 + 1)
def _image_loaders(put):
    out = []
    for (H, W), (Ho, Wo), clip in ((IMAGES[0], (19, 27), (1, 2, 3, 1)), (IMAGES[1], (1, 1), (0, 0, 0, 0))):
        imgs, masks = put(_u8((2, H, W, 3), H)), put(_u8((2, H, W), H + 1))
        out.append(ops.image_resize_u8(imgs, Ho, Wo, clip))
        out.append(ops.image_resize_mask_u8(imgs, masks, Ho, Wo, clip))
    out.append(ops.image_undistort_u8(put(_u8((2, 37, 53, 3), 5)), "OPENCV", (40.0, 41.0, 26.0, 18.0, 0.1, -0.02, 0.001, -0.002),
                                      (38.0, 38.0, 25.5, 17.7), 35, 51))
    out.append(ops.image_undistort_u8(put(_u8((1, 1, 1, 1), 6)), "SIMPLE_PINHOLE", (1.0, 0.5, 0.5), (1.0, 1.0, 0.5, 0.5), 1, 1))
    m_inv = np.linalg.inv(np.array([[1.2, 0.0, 0.1, 0.0], [0.0, 1.1, -0.1, 0.0], [0.0, 0.0, 1.0, 0.2], [0.0, 0.0, 0.0, 1.0]], np.float32))
    out.append(ops.pixel_rays(m_inv, 37, 53, (0.1, 0.2, -0.3), DEV))
    out.append(ops.pixel_rays(m_inv, 2, 2, None, DEV))
    rows = put(400.0 + 300.0 * torch.rand(80, 110, generator=_gen(8)))
    out.append(ops.depth_gt_prepare(rows, True, 2, 1, 37, 53, 1.0 / 320.7, put(0.8 + 0.2 * torch.rand(37 * 53, generator=_gen(9), dtype=torch.float64))))
    return out


@case("view_pair_scores", ["view_pair_scores"], allocs=2 * 2, refuses=["ufr_view_pair_scores"])
def _view_pair_scores(put):
    out = []
    for lengths in ((1, 65, 257), (4097, 5)):
        rng = np.random.default_rng(sum(lengths))
        M = 97
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        obs = rng.integers(-1, M, int(offsets[-1])).astype(np.int32)
        points = put(torch.from_numpy(rng.normal(size=(M, 3))))
        centres = put(torch.from_numpy(rng.normal(size=(len(lengths), 3)) * 0.3 + np.array([0.0, 0.0, -6.0])))
        out.append(ops.view_pair_scores(offsets, obs, points, centres, device=DEV))
    return out


# ------------------------------------------------------------------------------------------------------------- training
@case("adam", ["adam_step", "AdamTable", "optim.Adam"], allocs=2 * 3, modules=("ops", "optim"))
def _adam(put):
    numels = (1, 3, 4097)
    params, grads = TR.adam_case(numels, never=False, skip=None)
    ps, ms, vs = ([put(t) for t in params], [put(torch.zeros(n)) for n in numels], [put(torch.zeros(n)) for n in numels])
    for s in range(2):
        ops.adam_step(ps, [put(g) for g in grads[s]], ms, vs, [1 - 0.9 ** (s + 1)] * 3, [1 - 0.999 ** (s + 1)] * 3, 1e-3)
    qs = [put(t).requires_grad_(True) for t in params]
    opt = optim.Adam(qs, lr=1e-3)
    for s in range(2):
        for q, g in zip(qs, grads[s]):
            q.grad = put(g)
        opt.step()
    return ps, ms, vs, [q.detach() for q in qs], [opt.state[q]["exp_avg"] for q in qs], [opt.state[q]["exp_avg_sq"] for q in qs]


@case("select_rays", ["select_rays"], allocs=3 * 2, refuses=["ufr_select_rays"])
def _select_rays(put):
    return [ops.select_rays(put(TR.quantised_uniforms(n, seed=n)), k) for n, k in ((1, 1), (1961, 7), (5000, 4096))]


def GRAD_TOL():
    import test_gpu_backward

    return test_gpu_backward.GRAD_TOL


@case("autograd_training_step", ["autograd.RenderTwoPass", "autograd.RenderLoss", "render_loss", "composite_bwd", "project_gather_bwd"],
      allocs=12, modules=("ops", "autograd"))
def _training_step(put):
    import argparse

    from uforecon_amd import model as M

    fr = make_frame(32, 48, 3, seed=2, train_layout=True)
    RN = 5
    idx = (torch.arange(RN) * 83 + 120)[None]
    U1, U2 = sampler_uniforms(2, 32, 32, RN)
    args = argparse.Namespace(extract_geometry=False, coarse_sample=32, fine_sample=32, test_sample_coarse=32, test_sample_fine=32)
    m = M.UFORecon(args).to(DEV)
    m.load_state_dict(load_weights(), strict=True)
    batch = put.tree(fr.batch)
    r = m.infer(batch, put(idx), put(fr.source_imgs_feat), put.tree(fr.feature_volume), match_feature=put.tree(fr.match_feature),
                uniforms=(U1, U2))
    loss, _ = m.training_loss(r, batch)
    loss.backward()
    assert ops.status_poll(True) == 0
    grads = {k: Atomic(p.grad, GRAD_TOL()) for k, p in m.named_parameters() if p.grad is not None}
    assert grads
    return loss.detach(), r[1].detach(), r[2].detach(), r[8].detach(), r[9].detach(), grads


@case("autograd_nodes", ["autograd.RenderPass", "autograd.Aggregate", "autograd.Composite"], allocs=30, modules=("ops", "autograd"))
def _autograd_nodes(put):
    """the single-pass node, the reference-shaped aggregate and the compositor, each forwards and backwards at RN 5"""
    NV, RN, SN = 3, 5, 16
    P = RN * SN
    fr = FR.frame(NV)
    vols = [t.requires_grad_(True) for t in autograd.flat_volumes(put.tree(fr.feature_volume))]
    volumes = {st: dict(feature_volume=vols[2 * i], weight_volume=vols[2 * i + 1]) for i, st in enumerate(autograd.STAGES)}
    fh = ops.FrameHandle(put.tree(fr.batch), put(fr.source_imgs_feat), volumes, put.tree(fr.match_feature))
    raw = {k: put(v).requires_grad_("depthcode" not in k) for k, v in load_weights().items()}
    W = ops.PackedWeights(raw)
    params = [raw[k] for k in ops.RAW_WEIGHT_KEYS]
    o, d, z = _rays(put, NV, RN, SN)
    cot = lambda *shape: put(_rand(shape, sum(shape)))

    def grads_of(tensors, keys):
        out = {}
        for k, t in zip(keys, tensors):
            if t.grad is not None:
                bound = (FR.COMPOSITE_BOUNDS["d_variance"], _rel_scalar) if k.endswith("variance") else (ATOMICS(), grad_rel_err)
                out[k] = Atomic(t.grad.clone(), *bound)
                t.grad = None
        return out

    rgb, depth, opacity, weight, srdf, xy = autograd.RenderPass.apply(fh, W, o, d, z, *params, *vols)
    ((rgb * cot(RN, 3)).sum() + (depth * cot(RN)).sum() + (opacity * cot(RN)).sum() + (weight * cot(RN, SN)).sum()).backward()
    assert ops.status_poll(True) == 0
    import test_gpu_gather

    out = [(rgb.detach(), depth.detach(), opacity.detach(), weight.detach(), srdf.detach(), xy, grads_of(params, ops.RAW_WEIGHT_KEYS),
            [Atomic(v.grad.clone(), gather_ref.CAP_GRAD, test_gpu_gather._grad_err) for v in vols])]
    _, _, _, dbg = ops.project_gather(fh, W, o, d, z, debug=True)
    vol24 = dbg["vol24"].requires_grad_(True)
    radiance, srdf, xy = autograd.Aggregate.apply(fh, W, ops.points(o, d, z).reshape(P, 3), RN, SN, vol24, dbg["sim8"], *params)
    ((radiance * cot(P, 3)).sum() + (srdf * cot(RN, SN)).sum()).backward()
    assert ops.status_poll(True) == 0
    out.append((radiance.detach(), srdf.detach(), xy, vol24.grad, grads_of(params, ops.RAW_WEIGHT_KEYS)))
    c = {k: put(v) for k, v in FR.composite_inputs(17, 5).items()}
    rad, sd, var = c["radiance"].requires_grad_(True), c["srdf"].requires_grad_(True), put(torch.tensor(0.3)).requires_grad_(True)
    res = autograd.Composite.apply(c["z"], rad, sd, var)
    sum((r * c[k]).sum() for r, k in zip(res, ("d_rgb", "d_depth", "d_opacity", "d_weight"))).backward()
    out.append(([r.detach() for r in res], rad.grad, sd.grad, Atomic(var.grad, FR.COMPOSITE_BOUNDS["d_variance"], _rel_scalar)))
    return out


# ------------------------------------------------------------------------------------------------------------ the tests
def _flatten(out, key="out"):
    """[(key, host tensor or Atomic of one)] of a nested result"""
    if out is None:
        return [(key, None)]
    if isinstance(out, Atomic):
        return [(key, Atomic(out.t.detach().cpu().clone(), out.bound, out.err))]
    if torch.is_tensor(out):
        return [(key, out.detach().cpu().clone())]
    if isinstance(out, dict):
        return [kv for k in sorted(out) for kv in _flatten(out[k], f"{key}.{k}")]
    if isinstance(out, (list, tuple)):
        return [kv for i, v in enumerate(out) for kv in _flatten(v, f"{key}[{i}]")]
    if isinstance(out, (bool, int, float, str)):
        return [(key, out)]
    raise TypeError(f"{key}: {type(out)}")


def _same_bits(a, b) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _compare(name, clean, guarded):
    assert [k for k, _ in clean] == [k for k, _ in guarded], name
    bad = []
    for (k, a), (_, b) in zip(clean, guarded):
        if isinstance(a, Atomic):
            e = a.err(b.t, a.t) if a.t.numel() else 0.0
            if not e < a.bound:
                bad.append(f"{k}: differs by {e:.3e} of its scale (float atomics: bound {a.bound:.1e})")
        elif torch.is_tensor(a):
            if not _same_bits(a, b):
                where = "" if a.shape != b.shape or a.dtype != b.dtype else f", {int((a != b).sum())} of {a.numel()} elements"
                bad.append(f"{k}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}{where}")
        elif a != b and not (isinstance(a, float) and a != a and b != b):
            bad.append(f"{k}: {a!r} against {b!r}")
    assert not bad, f"{name}: the guarded run differs from the plain one (a result that depends on memory outside its tensors):\n  " + \
        "\n  ".join(bad)


def _run(c, guard=None):
    clear_caches()
    out = c.fn(Put(guard))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_guard_bands(name, monkeypatch):
    c = CASES[name]
    clean = _flatten(_run(c))
    guard = GuardedTorch().install(monkeypatch, *(MODULES[m] for m in c.modules))
    try:
        out = _run(c, guard)
        guard.check()
        print(f"GUARD {name}: {guard.guarded} allocations and {guard.placed} inputs between guards (declared: at least {c.allocs})")
        assert guard.guarded >= c.allocs, (name, guard.guarded, c.allocs)
        _compare(name, clean, _flatten(out))
    finally:
        clear_caches()          # a failing case leaves no guarded buffer in the wrappers' caches for the tests after it


# ----------------------------------------------------------------------------------------------- workspace refusals
def workspace_entry_points(header=HEADER):
    """{entry point: index of its ``workspace_bytes`` argument, or None where the count travels in ufr_render_args}, read from
    the prototypes of include/ufr.h"""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = {}
    for m in re.finditer(r"\bint\s+(ufr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        params = [p.strip() for p in m.group(2).split(",")]
        names = [re.findall(r"\w+", p)[-1] if re.findall(r"\w+", p) else "" for p in params]
        if "workspace_bytes" in names:
            found[m.group(1)] = names.index("workspace_bytes")
        elif any("ufr_render_args" in p for p in params):
            found[m.group(1)] = None
    return found


REFUSALS = {entry: c.name for c in CASES.values() for entry in c.refuses}


# The four entry points for which include/ufr.h states that a workspace that is too small is UFR_ERR_ARG (-1), not
# UFR_ERR_WORKSPACE (-3), and whose own tests pin that code (tests/test_gpu_raster.py, test_gpu_points.py, test_gpu_color_mesh.py,
# test_gpu_view_select.py).  The text is the same everywhere, and so is what matters here: refused before anything is written.
REFUSED_AS_ARGUMENT = {"ufr_raster_frames": -1, "ufr_splat_frames": -1, "ufr_color_vertices": -1, "ufr_view_pair_scores": -1}


class ShortWorkspace:
    """libufr as ``_lib.load()`` returns it, except that the first call of ``entry`` is given one byte less of workspace than
    the wrapper asked the library for; what the guarded buffers held just before that call is kept"""

    def __init__(self, real, entry, index, guard):
        self._real, self._entry, self._index, self._guard = real, entry, index, guard
        self.asked = self.rc = self.before = None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != self._entry or self.asked is not None:
            return fn

        def short(*args):
            args = list(args)
            if self._index is None:
                a = args[0]._obj                          # ufr_render_args, passed with byref
                self.asked = int(a.workspace_bytes)
                a.workspace_bytes = self.asked - 1
            else:
                self.asked = int(args[self._index])
                args[self._index] = self.asked - 1
            self.before = self._guard.snapshot()
            self.rc = fn(*args)
            return self.rc
        return short


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_short_workspace_is_refused_before_anything_is_written(entry, monkeypatch):
    c = CASES[REFUSALS[entry]]
    index = workspace_entry_points()[entry]
    guard = GuardedTorch().install(monkeypatch, *(MODULES[m] for m in c.modules))
    lib = ShortWorkspace(_lib.load(), entry, index, guard)
    monkeypatch.setattr(_lib, "_lib", lib)
    clear_caches()
    with pytest.raises(_lib.UfrError) as e:
        c.fn(Put(guard))
    clear_caches()
    assert lib.asked is not None and lib.asked > 0, f"{entry}: the case never called it"
    code = REFUSED_AS_ARGUMENT.get(entry, -3)                                         # UFR_ERR_WORKSPACE
    assert lib.rc == code, (entry, lib.rc)
    assert f"({code})" in str(e.value) and f": workspace too small: {lib.asked - 1} < {lib.asked} bytes" in str(e.value), str(e.value)
    guard.check()
    changed = guard.changed(lib.before)
    assert not changed, f"{entry}: refused, yet {len(changed)} buffer(s) were written:\n  " + "\n  ".join(changed)
