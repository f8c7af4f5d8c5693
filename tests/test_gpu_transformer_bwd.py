"""The per-ray transformers' backward stage by stage against float64 autograd through the oracle (tests/bwd_ref.py).

ufr_view_transform_bwd and ufr_ray_transform_bwd are checked on their own, at every view count, at point counts around
the view tape block, at every ray-tile shape class, with forced masks, in both matrix precisions; the forward-recorded
tape against the backward-built one and the stages one by one against STAGE_ALL; and a backward whose packed weights
were refitted to a frame with a far larger feature bound between its forward and its backward.

fp32 mode: element-wise |g - g64| <= EPS * scale + env, env = the ReLU-flip envelope (bwd_ref).  16-bit mode (one bf16
plane per operand): a per-tensor median and max bound, and it must sit measurably further from float64 than fp32 mode.
"""
import argparse
import copy

import pytest
import torch

import bwd_ref as R
from helpers import CASES, case_inputs, grad_rel_err, load_weights
from oracle import ufo_oracle as O
from uforecon_amd import model as M
from uforecon_amd import ops
from uforecon_amd.scene import make_frame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32, LOWP = ops.PRECISION_FP32, ops.PRECISION_16BIT

EPS = R.EPS          # fp32 mode, of each gradient tensor's scale outside the flip envelope (R.EPS_SUM: head biases)
MED16 = 3e-2         # 16-bit mode: per-tensor median of |g - g64| / scale (measured worst 1.6e-2) ...
MAX16 = 5e-1         # ... and its maximum (measured worst 0.25: d_token0 at SN = 256; bf16 operands, 8 significand bits)
FURTHER16 = 10.0     # 16-bit mode's worst tensor is at least this many times fp32 mode's
ATOMICS = 1e-6       # two runs that differ only in the order of float atomics, of each tensor's scale


def _gathered(NV, RN, SN, seed=0, feat_scale=1.0):
    """(W, fh, x, rgbm, dirs) of RN rays x SN samples of a seeded training-layout frame, through the HIP gather."""
    fr = make_frame(48, 64, NV, seed=40 + NV, train_layout=True)
    if feat_scale != 1.0:
        fr = copy.deepcopy(fr)
        fr.source_imgs_feat = fr.source_imgs_feat * feat_scale
        for st in fr.feature_volume:
            fr.feature_volume[st]["feature_volume"] = fr.feature_volume[st]["feature_volume"] * feat_scale
    W = ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})
    f = fr.to(DEV)
    fh = ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)
    g = torch.Generator().manual_seed(100 + seed)
    idx = torch.randperm(48 * 64, generator=g)[:RN]
    ray_d = fr.batch["ray_d"][0][:, idx].t().contiguous().to(DEV)
    ray_o = fr.batch["ray_o"][0].contiguous().to(DEV)
    near = fr.batch["near_fars"][0, 0, 0].expand(RN).contiguous().to(DEV)
    far = fr.batch["near_fars"][0, 0, 1].expand(RN).contiguous().to(DEV)
    z = ops.sample_fixed(near, far, torch.rand(SN, RN, generator=g).to(DEV))
    x, rgbm, dirs, _ = ops.project_gather(fh, W, ray_o, ray_d, z)
    return W, fh, x, rgbm, dirs


def _rand(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.5).to(DEV)


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _rel16(g, ref):
    """(median, max) of |g - g64| / scale over the tensor's elements (scale floor as helpers.grad_rel_err)"""
    d = (torch.as_tensor(g).double().cpu().reshape(ref.shape) - ref).abs().reshape(-1) / max(float(ref.abs().max()), R.FLOOR)
    return float(d.median()), float(d.max())


def _check_modes(label, e, run):
    """run(precision) -> {name: kernel gradient}.  fp32 mode inside the envelope at EPS; 16-bit mode within MED16 / MAX16
    and FURTHER16 times further from float64 than fp32 mode.  Returns the fp32 gradients."""
    g32 = run(FP32)
    ex = e.excesses(g32)
    g16 = run(LOWP)
    rel16 = {k: _rel16(v, e.g_nom[k]) for k, v in g16.items() if k != R.SHIFT_BIAS}
    w32, w16 = max(ex, key=ex.get), max(rel16, key=lambda k: rel16[k][1])
    med16 = max(v[0] for v in rel16.values())
    print(f"MEASURE {label}: |A| {len(e.ambiguous)}  fp32 worst {ex[w32]:.2e} ({w32})  16-bit worst {rel16[w16][1]:.2e} "
          f"({w16}) worst median {med16:.2e}")
    bad = e.beyond(g32)
    assert not bad, (label, bad)
    if R.SHIFT_BIAS in g32:
        assert e.check_shift_bias(g32[R.SHIFT_BIAS]) and e.check_shift_bias(g16[R.SHIFT_BIAS], rel=MAX16)
    assert med16 < MED16 and rel16[w16][1] < MAX16, (label, rel16)
    w32 = max((v for k, v in ex.items() if k not in R.SUM_KEYS), default=0.0)
    assert rel16[w16][1] > FURTHER16 * max(w32, 1e-7), (label, rel16[w16][1], w32)   # the 16-bit mode applied
    return g32


def _grads_of(grads, keys):
    return {k: grads.grad(k).detach().cpu().clone() for k in keys}


# ------------------------------------------------------------------ view transformer backward
def _view_inputs(NV, P, masks):
    """P points of gathered tokens; masks: 'gathered' as they come, 'all_masked' = every view masked on every other
    point (all P when P == 1), 'one_unmasked' = exactly one view unmasked on every other point."""
    W, _, x, rgbm, dirs = _gathered(NV, 2, 32, seed=NV)
    x, rgbm, dirs = x[:P].contiguous(), rgbm[:P].clone(), dirs[:P].contiguous()
    pts = torch.arange(0, P, 2, device=DEV)
    if masks == "all_masked":
        rgbm[pts, :, 3] = 0.0
    elif masks == "one_unmasked":
        rgbm[pts, :, 3] = 0.0
        rgbm[pts, pts % NV, 3] = 1.0
    return W, x, rgbm, dirs, pts


def _view_bwd(W, x, rgbm, dirs, ta, tb, dr, precision):
    grads = ops.GradBuffer(DEV)
    d_pv = ops.view_transform_bwd(W, grads, x, rgbm, dirs, ta, tb, dr, precision=precision)
    assert ops.status_poll(True) == 0
    out = _grads_of(grads, R.VIEW_KEYS)
    out["d_pv"] = d_pv.cpu()
    return out


def _view_env(x, rgbm, dirs, ta, tb, dr):
    t0 = None if ta is None else _cpu(ta) + (0 if tb is None else _cpu(tb))
    return R.view_envelope(load_weights(), x.cpu(), rgbm.cpu()[..., :3], rgbm.cpu()[..., 3], dirs.cpu()[..., :3], t0, _cpu(dr))


@pytest.mark.parametrize("masks", ["gathered", "all_masked", "one_unmasked"])
@pytest.mark.parametrize("pcase", ["1", "B-1", "B", "B+1", "3B+B/2"])
@pytest.mark.parametrize("NV", [2, 3, 4, 5, 6, 7])
def test_view_bwd_against_float64(NV, pcase, masks):
    B = ops.view_tape_block_points(NV)
    P = {"1": 1, "B-1": B - 1, "B": B, "B+1": B + 1, "3B+B/2": 3 * B + B // 2}[pcase]
    W, x, rgbm, dirs, pts = _view_inputs(NV, P, masks)
    ta, tb, dr = _rand((P, 80), 1), _rand((P, 80), 2), _rand((P, 3), 3)
    e = _view_env(x, rgbm, dirs, ta, tb, dr)
    g32 = _check_modes(f"view NV={NV} P={P} {masks}", e, lambda prec: _view_bwd(W, x, rgbm, dirs, ta, tb, dr, prec))
    if masks == "all_masked":
        # the logit gradient of a point whose views are all masked goes to the -1e9 constant (torch.where): its
        # d_radiance reaches no parameter and no d_pv row
        dr0 = dr.clone()
        dr0[pts] = 0.0
        g0 = _view_bwd(W, x, rgbm, dirs, ta, tb, dr0, FP32)
        for k in g32:
            if k != R.SHIFT_BIAS:      # (rounding noise on both sides)
                assert grad_rel_err(g0[k], g32[k]) < ATOMICS, k


@pytest.mark.parametrize("NV", [2, 3, 4, 5, 6, 7])
def test_view_bwd_optional_cotangents(NV):
    """NULL d_token0_b (one partial buffer) is allowed; the data-gradient stage refuses a NULL d_radiance."""
    from uforecon_amd._lib import UfrError

    P = ops.view_tape_block_points(NV) + 1
    W, x, rgbm, dirs, _ = _view_inputs(NV, P, "gathered")
    ta, dr = _rand((P, 80), 4), _rand((P, 3), 6)
    e = _view_env(x, rgbm, dirs, ta, None, dr)
    _check_modes(f"view NV={NV} P={P} no d_token0_b", e, lambda prec: _view_bwd(W, x, rgbm, dirs, ta, None, dr, prec))
    with pytest.raises(UfrError):
        ops.view_transform_bwd(W, ops.GradBuffer(DEV), x, rgbm, dirs, ta, None, None)


# ------------------------------------------------------------------ ray transformer backward
def _ray_inputs(RN, SN, seed=0):
    W, _, x, rgbm, dirs = _gathered(3, RN, SN, seed=seed)
    token0, _ = ops.view_transform(W, x, rgbm, dirs, precision=FP32)
    return W, token0, _rand((RN, SN), 7 + SN)


def _ray_bwd(W, token0, RN, SN, d_srdf, precision):
    grads = ops.GradBuffer(DEV)
    a, b = ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, precision=precision)
    assert ops.status_poll(True) == 0
    out = _grads_of(grads, R.RAY_KEYS)
    out["d_token0"] = (a + b).cpu()
    return out


@pytest.mark.parametrize("SN,RN", [(16, 37), (32, 37), (32, 3), (80, 3), (112, 3), (128, 1), (128, 3), (240, 1),
                                   (256, 1), (256, 3)])
def test_ray_bwd_against_float64(SN, RN):
    """Every tile-count class of the ray kernel: one tile (16), even and odd tile counts (80, 112, 240: a padding tile in
    the last block), the API's largest SN (256); several rays per launch."""
    W, token0, d_srdf = _ray_inputs(RN, SN)
    e = R.ray_envelope(load_weights(), token0.cpu(), RN, SN, d_srdf.cpu())
    _check_modes(f"ray SN={SN} RN={RN}", e, lambda prec: _ray_bwd(W, token0, RN, SN, d_srdf, prec))


def test_ray_bwd_pool_form_equals_plain_form_scattered():
    """row / accumulate: slot (ray, s) reads and writes pool row row[ray, s] and adds onto what the buffers hold; rows no
    slot names stay untouched.  The same kernel arithmetic as the plain form on the gathered rows: bit-identical d_token0;
    the weight gradients differ only by the order of the float atomics."""
    RN, SN, M_ = 3, 80, 400
    W, token0, d_srdf = _ray_inputs(RN, SN, seed=1)
    g = torch.Generator().manual_seed(9)
    row = torch.randperm(M_, generator=g)[:RN * SN].reshape(RN, SN).to(torch.int32).to(DEV)
    pool = _rand((M_, 80), 10)
    pool[row.reshape(-1).long()] = token0
    pa, pb = _rand((M_, 80), 11), _rand((M_, 80), 12)
    a0, b0 = pa.clone(), pb.clone()
    gp = ops.GradBuffer(DEV)
    ops.ray_transform_bwd(W, gp, pool, RN, SN, d_srdf, row=row, out=(pa, pb), accumulate=True, precision=FP32)
    gplain = ops.GradBuffer(DEV)
    a, b = ops.ray_transform_bwd(W, gplain, token0, RN, SN, d_srdf, precision=FP32)
    assert ops.status_poll(True) == 0
    r = row.reshape(-1).long()
    unused = torch.ones(M_, dtype=torch.bool, device=DEV)
    unused[r] = False
    assert torch.equal(pa[unused], a0[unused]) and torch.equal(pb[unused], b0[unused])
    # each pool row is the buffer's content plus the plain form's value (one fp32 add: compared at that rounding)
    assert grad_rel_err(pa[r] + pb[r], (a0[r] + a) + (b0[r] + b)) < ATOMICS
    for k in R.RAY_KEYS:
        assert grad_rel_err(gp.grad(k), gplain.grad(k)) < ATOMICS, k


# ------------------------------------------------------------------ aggregate chain, tapes and stages
def _chain(W, x, rgbm, dirs, RN, SN, d_rad, d_srdf, precision, mode, chunks=None):
    """Both backwards chained (ray -> view).  mode 'all': STAGE_ALL; 'stages': TAPE, DGRAD, WGRAD as separate calls on one
    workspace; 'forward_tape': the tape recorded by view_transform_tape over ``chunks`` + ray_transform_tape, the
    backward from DGRAD.  -> ({name: gradient}, token0, radiance, srdf of the forward)."""
    P, NV = x.shape[0], x.shape[1]
    grads = ops.GradBuffer(DEV)
    vws = ops.view_transform_bwd_workspace(P, NV, DEV)
    rws = ops.ray_transform_bwd_workspace(RN, SN, DEV)
    if mode == "forward_tape":
        token0 = torch.empty(P, 80, device=DEV)
        radiance = torch.empty(P, 3, device=DEV)
        for p0, p1 in chunks:
            ops.view_transform_tape(W, x[p0:p1], rgbm[p0:p1], dirs[p0:p1], token0[p0:p1], radiance[p0:p1], vws, p0, P,
                                    precision=precision)
        srdf = ops.ray_transform_tape(W, token0, RN, SN, rws, precision=precision)
        first = ops.STAGE_DGRAD
    else:
        token0, radiance = ops.view_transform(W, x, rgbm, dirs, precision=precision)
        srdf = ops.ray_transform(W, token0, RN, SN, precision=precision)
        first = ops.STAGE_TAPE | ops.STAGE_DGRAD
    if mode == "stages":
        a, b = ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, precision=precision, stages=ops.STAGE_TAPE, workspace=rws)
        ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, out=(a, b), precision=precision, stages=ops.STAGE_DGRAD,
                              workspace=rws)
        ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, out=(a, b), precision=precision, stages=ops.STAGE_WGRAD,
                              workspace=rws)
        ops.view_transform_bwd(W, grads, x, rgbm, dirs, None, None, None, precision=precision, stages=ops.STAGE_TAPE,
                               workspace=vws)
        d_pv = ops.view_transform_bwd(W, grads, x, rgbm, dirs, a, b, d_rad, precision=precision, stages=ops.STAGE_DGRAD,
                                      workspace=vws)
        ops.view_transform_bwd(W, grads, x, rgbm, dirs, None, None, None, precision=precision, stages=ops.STAGE_WGRAD,
                               workspace=vws)
    else:
        rest = ops.STAGE_WGRAD | (first if mode == "forward_tape" else ops.STAGE_ALL)
        a, b = ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, precision=precision, stages=rest, workspace=rws)
        d_pv = ops.view_transform_bwd(W, grads, x, rgbm, dirs, a, b, d_rad, precision=precision, stages=rest, workspace=vws)
    assert ops.status_poll(True) == 0
    out = _grads_of(grads, R.VIEW_KEYS + R.RAY_KEYS)
    out["d_pv"], out["d_token0"] = d_pv.cpu(), (a + b).cpu()
    return out, token0.cpu(), radiance.cpu(), srdf.cpu()


def _agg_env(x, rgbm, dirs, RN, SN, d_rad, d_srdf):
    return R.grad_envelope(load_weights(), x.cpu(), rgbm.cpu()[..., :3], rgbm.cpu()[..., 3], dirs.cpu()[..., :3], RN, SN,
                           d_rad.cpu(), d_srdf.cpu())


def _same(label, ref, other):
    """forward rows and data gradients bit-identical; weight gradients up to the order of the float atomics"""
    g0, t0, r0, s0 = ref
    g1, t1, r1, s1 = other
    assert torch.equal(t0, t1) and torch.equal(r0, r1) and torch.equal(s0, s1), label
    diff = {k: grad_rel_err(g1[k], g0[k]) for k in g0}
    print(f"MEASURE {label}: largest difference {max(diff.values()):.1e}; bit-identical data gradients "
          f"{torch.equal(g0['d_pv'], g1['d_pv']) and torch.equal(g0['d_token0'], g1['d_token0'])}")
    bad = {k: v for k, v in diff.items() if not v < ATOMICS}
    assert not bad, (label, bad)


@pytest.mark.parametrize("precision", [FP32, LOWP])
@pytest.mark.parametrize("NV", [2, 6, 7])
def test_forward_tape_and_stages_equal_the_backward_built_tape(NV, precision):
    """A tape recorded by the training forward (view tape in chunks of whole tape blocks, the last one closing the pool,
    + the ray tape) gives what the backward's own tape stage gives, and so do the three stages run one by one.  The
    forward rows and data gradients are bit-identical (same kernels, same arithmetic, no atomics); the weight gradients are
    float atomics whose order may differ: bounded by ATOMICS."""
    RN, SN = 3, 48
    B = ops.view_tape_block_points(NV)
    W, _, x, rgbm, dirs = _gathered(NV, RN, SN, seed=20 + NV)
    P = RN * SN
    cuts = [0, B, 5 * B, (P // (2 * B)) * B, P]
    chunks = list(zip(cuts[:-1], cuts[1:]))
    d_rad, d_srdf = _rand((P, 3), 21), _rand((RN, SN), 22)
    built = _chain(W, x, rgbm, dirs, RN, SN, d_rad, d_srdf, precision, "all")
    _same(f"NV={NV} prec={precision} forward tape", built, _chain(W, x, rgbm, dirs, RN, SN, d_rad, d_srdf, precision,
                                                                   "forward_tape", chunks))
    _same(f"NV={NV} prec={precision} stages", built, _chain(W, x, rgbm, dirs, RN, SN, d_rad, d_srdf, precision, "stages"))
    if precision == FP32:
        e = _agg_env(x, rgbm, dirs, RN, SN, d_rad, d_srdf)
        ex = e.excesses(built[0])
        print(f"MEASURE aggregate chain NV={NV}: |A| {len(e.ambiguous)} worst {max(ex.values()):.2e} ({max(ex, key=ex.get)})")
        assert not e.beyond(built[0]), ex


# ------------------------------------------------------------------ scale-table refit between forward and backward
def test_refit_between_forward_and_backward_keeps_the_float64_bound():
    """ufr_weights_fit_frame (include/ufr.h): a frame with features x 1e4 lowers the activation exponents of a packed blob
    that a frame A forward has already used.  A's backward -- from the tape its forward recorded, and with STAGE_TAPE
    recomputing under the new table -- meets the same float64 bound as without the refit."""
    NV, RN, SN = 3, 3, 32
    W, fhA, x, rgbm, dirs = _gathered(NV, RN, SN, seed=30)
    P = RN * SN
    chunks = [(0, P)]
    d_rad, d_srdf = _rand((P, 3), 31), _rand((RN, SN), 32)
    e = _agg_env(x, rgbm, dirs, RN, SN, d_rad, d_srdf)
    before = _chain(W, x, rgbm, dirs, RN, SN, d_rad, d_srdf, FP32, "all")
    # A's training forward records its tape under the table fitted to A ...
    grads = ops.GradBuffer(DEV)
    vws, rws = ops.view_transform_bwd_workspace(P, NV, DEV), ops.ray_transform_bwd_workspace(RN, SN, DEV)
    token0, radiance = torch.empty(P, 80, device=DEV), torch.empty(P, 3, device=DEV)
    ops.view_transform_tape(W, x, rgbm, dirs, token0, radiance, vws, 0, P, precision=FP32)
    ops.ray_transform_tape(W, token0, RN, SN, rws, precision=FP32)
    a_before = W.scale_exponents()["vt_q"][1]
    # ... then the same blob is fitted to frame B
    _, fhB, *_ = _gathered(NV, RN, SN, seed=30, feat_scale=1e4)
    W.fit(fhB)
    a_after = W.scale_exponents()["vt_q"][1]
    assert a_after < a_before, (a_before, a_after)
    rest = ops.STAGE_DGRAD | ops.STAGE_WGRAD
    a, b = ops.ray_transform_bwd(W, grads, token0, RN, SN, d_srdf, precision=FP32, stages=rest, workspace=rws)
    d_pv = ops.view_transform_bwd(W, grads, x, rgbm, dirs, a, b, d_rad, precision=FP32, stages=rest, workspace=vws)
    assert ops.status_poll(True) == 0
    taped = _grads_of(grads, R.VIEW_KEYS + R.RAY_KEYS)
    taped["d_pv"], taped["d_token0"] = d_pv.cpu(), (a + b).cpu()
    recomputed = _chain(W, x, rgbm, dirs, RN, SN, d_rad, d_srdf, FP32, "all")[0]
    res, bad = {}, {}
    for label, g in (("no refit", before[0]), ("forward tape after refit", taped), ("recomputed after refit", recomputed)):
        res[label] = max(e.excesses(g).values())
        bad[label] = e.beyond(g)
        assert e.check_shift_bias(g[R.SHIFT_BIAS]), label
    print(f"MEASURE refit: a(vt_q) {a_before} -> {a_after}; |A| {len(e.ambiguous)}; worst excess {res}")
    assert not any(bad.values()), bad


def _args(c):
    return argparse.Namespace(extract_geometry=False, test_sample_coarse=c["coarse"], test_sample_fine=c["fine"],
                              coarse_sample=c["coarse"], fine_sample=c["fine"], volume_type="correlation", volume_reso=96,
                              mvs_depth_guide=1, depth_pos_encoding=True, use_dir_srdf=False, explicit_similarity=True,
                              test_coarse_only=False, test_ray_num=800)


@pytest.mark.parametrize("tape_in_forward", [True, False])
def test_model_refit_between_two_forwards_and_one_backward(tape_in_forward):
    """UFORecon.infer on frame A, then on frame B (features x 1e4: the shared packed weights are refitted), then one
    backward: (L_A + L_B) matches A and B each backpropagated on a fresh model, and L_A alone after B's forward matches
    A on a fresh model -- at the joint-vs-separate bound of test_two_forwards_before_one_backward_keep_their_own_tapes."""
    name = "c5_train_grads"
    c = CASES[name]
    frA, idx, U1, U2, _ = case_inputs(name)
    frB = copy.deepcopy(frA)
    frB.source_imgs_feat = frB.source_imgs_feat * 1e4
    for st in frB.feature_volume:
        frB.feature_volume[st]["feature_volume"] = frB.feature_volume[st]["feature_volume"] * 1e4
    fA, fB = frA.to(DEV), frB.to(DEV)

    def run(frames, weights_of_losses):
        m = M.UFORecon(_args(c), tape_in_forward=tape_in_forward).to(DEV)
        m.load_state_dict(load_weights(), strict=True)
        m.train()
        losses = []
        for f in frames:
            r = m.infer(f.batch, idx.to(DEV), f.source_imgs_feat, f.feature_volume, match_feature=f.match_feature,
                        uniforms=(U1, U2))
            losses.append(O.training_loss(dict(rgb=r[1][0], depth=r[2][0], rgb_2=r[8][0], depth_2=r[9][0]), f.batch,
                                          idx.to(DEV)))
        sum(w * l for w, l in zip(weights_of_losses, losses) if w).backward()
        torch.cuda.synchronize()
        assert ops.status_poll(True) == 0
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    gA, gB = run([fA], [1.0]), run([fB], [1.0])
    joint = run([fA, fB], [1.0, 1.0])
    a_only = run([fA, fB], [1.0, 0.0])
    worst = {}
    for k in gA:
        if k == R.SHIFT_BIAS:     # true gradient zero: rounding noise on every side
            continue
        worst[k] = (grad_rel_err(joint[k], gA[k] + gB[k]), grad_rel_err(a_only[k], gA[k]))
    print(f"MEASURE model refit tape_in_forward={tape_in_forward}: joint {max(v[0] for v in worst.values()):.1e} "
          f"A after B's forward {max(v[1] for v in worst.values()):.1e}")
    for k, (j, a) in worst.items():
        assert j < 2e-4 and a < 2e-4, (k, j, a)
