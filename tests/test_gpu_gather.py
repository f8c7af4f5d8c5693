"""The gather (ufr_project_gather) and its volume scatter (ufr_project_gather_bwd) against float64, at every view count.

gather.hip has one instantiation per view count NV = 2..7 whose LDS regions alias each other differently (the rows that
become token columns 32..71 lie over the footprints at NV <= 3 and inside the similarity slots at NV >= 4), a block -> XCD
remap that grids of fewer than 8 blocks and the tail blocks of other grids skip, a partial last block, two optional inputs
and per-ray origins; gather_bwd.hip folds equal voxel corners across lanes before it issues atomics.  Every case here runs
on ray sets that leave the source images, pass behind source cameras and leave every frustum (tests/gather_ref.py;
tests/test_gather_ref.py proves their shares), and is compared with the float64 oracle.

Bounds.  A quantity's yardstick is the fp32 oracle's own distance from float64 on the same inputs, computed here on the CPU
(never from the kernel's output); the kernel's bound is gather_ref.bound(yardstick, cap) = min(4 x yardstick, max(cap,
2 x yardstick)) with the suite's present caps: 1e-5 for rows, 5e-6 for xy, 1e-4 for gradients.  A cap is exceeded -- by the
second term only, i.e. at twice the yardstick -- where the fp32 restatement itself is farther than half the cap from
float64.  Largest yardsticks over the matrix: xy 4.4e-6, sim8 6.3e-5, vol24 / vol 1.8e-5, rgb 3.6e-5, feat 2.0e-5, sim16
1.4e-5 (all of these exceed half their cap on some set), dirs 5.3e-7, volume gradients 2.3e-5, pre_sim_mlp gradients
7.7e-7 (never).  Masks are compared exactly on every view-sample outside gather_ref.comparable's exclusion (at most 2 %
of a set, asserted on the CPU).  The depth encoding is bounded element by element: 4 x (2^k pi |delta32 - delta64| + an ulp)
plus, once and without the margin, a forward bound of delta's roundings (gather_ref.pe_tolerance: the first term alone is
no bound, and the kernel exceeds it by up to 2.54 x on a few elements of 20 of the 60 cases; the fp32 oracle reaches 0.13).

MEASURED on the MI355X, worst kernel error over the whole matrix as a fraction of its bound: xy, sim8, vol24, vol, feat, rgb 0.50
(the kernel's distance from float64 equals the fp32 oracle's to three digits: the same roundings), sim16 0.51, dirs 0.30
(1.7e-7 against a yardstick of 1.4e-7: the v_rcp), depth PE 0.155 of the element bound (NV 3, 27 x 24); masks exact.
Scatter, every form (plain, larger pool, permuted pool, accumulate): at most 0.28 of the bound in the last run; the
atomics' order varies from run to run, and an earlier run reached 0.78 (accumulate) and 0.72 (permuted pool).  pre_sim_mlp
gradients 3.5e-7 at worst against yardsticks of 1e-7..8e-7.
"""
import functools

import pytest
import torch

import gather_ref as G
from helpers import load_weights
from uforecon_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ST = G.STAGES


@pytest.fixture(scope="module")
def weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


@functools.lru_cache(maxsize=None)
def _frame(NV):
    fr = G.frame_for(NV)
    f = fr.to(DEV)
    return fr, ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)


@functools.lru_cache(maxsize=None)
def _pool_yardstick(NV):
    fr, _ = _frame(NV)
    RN, SN, per_ray = G.POOL_SHAPE
    o, d, z = G.offaxis_rays(fr, RN, SN, NV, per_ray)
    P = load_weights()
    return G.row_errors(G.rows(P, fr, o, d, z, torch.float32), G.rows(P, fr, o, d, z))


def _gather(fh, weights, o, d, z, **kw):
    """The kernel's outputs in the reference's shapes; x / rgb / dirs are handed over NaN-filled, and ops.project_gather
    NaN-fills the debug outputs itself, so a row the kernel does not write cannot pass by holding an earlier call's values."""
    RN, SN = z.shape
    NV, P = fh.NV, RN * SN
    out = tuple(torch.full((P, NV, c), float("nan"), device=DEV) for c in (80, 4, 4))
    x, rgbm, dirs, dbg = ops.project_gather(fh, weights, o.to(DEV), d.to(DEV), z.to(DEV).contiguous(), out=out, **kw)
    assert ops.status_poll(True) == 0
    got = dict(x=x.cpu(), rgb=rgbm[..., :3].cpu(), mask=rgbm[..., 3].cpu().reshape(RN, SN, NV).permute(2, 0, 1),
               dirs=dirs[..., :3].cpu(), dirs_pad=dirs[..., 3].cpu())
    for k, shape in (("xy", (NV, RN, SN, 2)), ("mask_z", (NV, RN, SN)), ("sim8", (RN, SN, 8)), ("vol24", (RN, SN, 24))):
        if k in dbg:
            got[k] = dbg[k].cpu().reshape(shape)
    return got


def _check_rows(tag, got, r32, r64, yard, fr, keys):
    """Every quantity in `keys` within its bound; masks exactly; the depth encoding element by element."""
    err = G.row_errors({**r32, **got}, r64)          # (quantities the kernel did not return fall back to r32: not asserted)
    frac = {}
    for k in keys:
        b = G.bound(yard[k], G.ROW_CAPS[k])
        frac[k] = err[k] / b
        print(f"GATHER {tag} {k}: kernel {err[k]:.2e} yardstick {yard[k]:.2e} bound {b:.2e}")
    cmp = G.comparable(r64)
    RN, SN = r64["sim8"].shape[:2]
    NV = fr.NV
    tol = G.pe_tolerance(fr, r32, r64)
    pe = got["x"][..., 72:80].double().reshape(RN, SN, NV, 8).permute(2, 0, 1, 3)
    pe64 = r64["x"][..., 72:80].reshape(RN, SN, NV, 8).permute(2, 0, 1, 3)
    frac["pe"] = float(((pe - pe64).abs() / tol).max())
    print(f"GATHER {tag} pe: worst element at {frac['pe']:.2f} of its bound")
    for k in keys:
        assert frac[k] < 1.0, (tag, k, err[k], yard[k])
    assert frac["pe"] <= 1.0, (tag, frac["pe"])
    if "mask_z" in got:
        assert torch.equal(got["mask_z"].double()[cmp], r64["mask_z"][cmp]), tag
    if "xy" in got:     # the in-image test on the kernel's own coordinates, behind the cameras (mask_z = 0) too
        kx = got["xy"].abs()
        assert torch.equal(((kx[..., 0] <= 1.) & (kx[..., 1] <= 1.)).double()[cmp], r64["inb"][cmp]), tag
    assert torch.equal(got["mask"].double()[cmp], r64["mask"][cmp]), tag           # in-image x in-front mask
    assert float(got["dirs_pad"].abs().max()) == 0.0
    return frac


@pytest.mark.parametrize("RN,SN,per_ray", G.FORWARD_SHAPES)
@pytest.mark.parametrize("NV", G.NVS)
def test_forward_rows_match_float64(NV, RN, SN, per_ray, weights):
    fr, fh = _frame(NV)
    P = load_weights()
    o, d, z = G.offaxis_rays(fr, RN, SN, NV, per_ray)
    r64, r32 = G.rows(P, fr, o, d, z), G.rows(P, fr, o, d, z, torch.float32)
    yard = G.yardstick(G.row_errors(r32, r64), _pool_yardstick(NV))
    got = _gather(fh, weights, o, d, z, debug=True)
    _check_rows(f"fwd NV{NV} {RN}x{SN} {'per-ray' if per_ray else 'one'} origin", got, r32, r64, yard, fr,
                ("xy", "sim8", "vol24", "feat", "vol", "sim16", "rgb", "dirs"))


@pytest.mark.parametrize("shape", G.SUPPLIED_SHAPES)
@pytest.mark.parametrize("NV", G.NVS)
def test_forward_with_supplied_lookup_and_similarity(NV, shape, weights):
    """vol24_in / sim8_in (RayTransformer.forward receives both as arguments): the supplied lookup arrives unchanged in
    columns 32..55 of every view's row, pre_sim_mlp of the supplied similarity in 56..71.  'aggregate' is the shape
    autograd.Aggregate calls: SN = 1, the points as per-ray origins, zero directions."""
    fr, fh = _frame(NV)
    P = load_weights()
    o, d, z = G.supplied_rays(fr, shape)
    RN, SN = z.shape
    g = torch.Generator().manual_seed(NV)
    vol24_in = (torch.rand(RN * SN, 24, generator=g) - 0.5) * 3.0
    sim8_in = torch.rand(RN * SN, 8, generator=g) * 2 - 1
    r64 = G.rows(P, fr, o, d, z, vol24_in=vol24_in, sim8_in=sim8_in)
    r32 = G.rows(P, fr, o, d, z, torch.float32, vol24_in=vol24_in, sim8_in=sim8_in)
    yard = G.yardstick(G.row_errors(r32, r64), {**_pool_yardstick(NV), "sim16": 0.0, "vol24": 0.0, "vol": 0.0, "sim8": 0.0})
    got = _gather(fh, weights, o, d, z, vol24_in=vol24_in.to(DEV), sim8_in=sim8_in.to(DEV), want_xy=True)
    for v in range(NV):
        assert torch.equal(got["x"][:, v, 32:56], vol24_in), v                      # unchanged, bit for bit
    _check_rows(f"supplied NV{NV} {shape}", got, r32, r64, yard, fr, ("xy", "feat", "sim16", "rgb", "dirs"))


# ------------------------------------------------------------------------------------------------------------- scatter
def _grad_err(a, b) -> float:
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _targets(fr, fill):
    shapes = [tuple(fr.feature_volume[st][k].shape) for st in ST for k in ("feature_volume", "weight_volume")]
    t = [fill(s) for s in shapes]
    return t, t[0::2], t[1::2]


def _scatter_case(NV, kind, RN, SN, per_ray):
    fr, fh = _frame(NV)
    P = load_weights()
    o, d, z = G.backward_rays(fr, kind, RN, SN, per_ray, NV)
    RN, SN = z.shape
    g = torch.Generator().manual_seed(100 * NV + SN)
    d_pv = torch.rand(RN * SN, 40, generator=g) - 0.5
    sim8 = G.rows(P, fr, o, d, z, torch.float32)["sim8"].reshape(-1, 8).contiguous()     # the fp32 oracle's: no kernel involved
    gv64, gp64 = G.scatter_grads(P, fr, o, d, z, sim8, d_pv)
    gv32, gp32 = G.scatter_grads(P, fr, o, d, z, sim8, d_pv, torch.float32)
    return fr, fh, o, d, z, d_pv, sim8, gv64, gp64, gv32, gp32, g


@pytest.mark.parametrize("kind,RN,SN,per_ray", G.BACKWARD_CASES)
@pytest.mark.parametrize("NV", G.NVS)
def test_scatter_matches_float64_autograd(NV, kind, RN, SN, per_ray, weights):
    """The six volume gradients as dense tensors (the zeros outside the touched voxels included) and the pre_sim_mlp
    parameter gradients against float64 autograd; the pool forms (`row=`) and accumulate=True within the same bounds."""
    fr, fh, o, d, z, d_pv, sim8, gv64, gp64, gv32, gp32, g = _scatter_case(NV, kind, RN, SN, per_ray)
    P = z.numel()
    tag = f"bwd NV{NV} {kind} {z.shape[0]}x{z.shape[1]}"
    bounds = [G.bound(_grad_err(a, b), G.CAP_GRAD) for a, b in zip(gv32, gv64)]
    # The pre_sim_mlp parameter gradients are ONE compared quantity: its yardstick is the largest over the six tensors.  Taken
    # per tensor it is degenerate: a bias gradient has 32 elements, each a sum over the points that torch adds pairwise, and
    # the fp32 oracle then lands within 0.7 ulp of float64 (8.6e-8 at NV 3, 27 x 24, pre_sim_mlp.0.bias).  No other summation
    # order of 648 fp32 terms can be held to 4 x that, and the kernel's (tiles of 32 points, then atomics) is not even fixed.
    yard_p = max(_grad_err(gp32[k], gp64[k]) for k in G.PRESIM_KEYS)
    bounds_p = {k: G.bound(yard_p, G.CAP_GRAD) for k in G.PRESIM_KEYS}
    dev = lambda t: t.to(DEV).contiguous()

    def check(form, got, grads, base=None):
        worst = 0.0
        for i, (a, ref) in enumerate(zip(got, gv64)):
            a = a.cpu().double() - (0 if base is None else base[i].cpu().double())
            e = _grad_err(a, ref)
            worst = max(worst, e / bounds[i])
            assert e < bounds[i], (tag, form, i, e, bounds[i])
            if base is None:      # a voxel no sample touches holds an exact zero, not a small number
                untouched = (ref == 0) & (gv32[i] == 0)
                assert float(a[untouched].abs().max()) == 0.0, (tag, form, i)
        for k in G.PRESIM_KEYS if grads is not None else ():
            e = _grad_err(grads.grad(k), gp64[k])
            worst = max(worst, e / bounds_p[k])
            assert e < bounds_p[k], (tag, form, k, e, bounds_p[k])
        print(f"GATHER {tag} {form}: worst at {worst:.2f} of its bound; volume bounds {min(bounds):.1e}..{max(bounds):.1e}, "
              f"pre_sim_mlp bounds {min(bounds_p.values()):.1e}..{max(bounds_p.values()):.1e}")

    # plain form, targets overwritten whole
    all_t, gf, gw = _targets(fr, lambda s: torch.full(s, 7.0, device=DEV))
    grads = ops.GradBuffer(DEV)
    ops.project_gather_bwd(fh, weights, grads, dev(o), dev(d), dev(z), dev(sim8), dev(d_pv), gf, gw, accumulate=False)
    assert ops.status_poll(True) == 0
    check("plain", all_t, grads)
    # pool form: slot (ray, s) owns row row[ray, s] of d_pv.  The volume scatter reads d_pv through `row` alone, so the pool
    # may be larger than the launch; the pre_sim_mlp half sums over the first RN*SN pool rows in any order (include/ufr.h:
    # the two-pass step's rows are a permutation of its pool), so it is checked on a pool that is exactly a permutation.
    for form, NP, presim in (("larger pool", 2 * P + 7, False), ("permuted pool", P, True)):
        row = torch.randperm(NP, generator=g)[:P]
        pool_d, pool_s = torch.rand(NP, 40, generator=g) - 0.5, torch.rand(NP, 8, generator=g)
        pool_d[row], pool_s[row] = d_pv, sim8
        all_t, gf, gw = _targets(fr, lambda s: torch.full(s, -3.0, device=DEV))
        grads = ops.GradBuffer(DEV)
        ops.project_gather_bwd(fh, weights, grads, dev(o), dev(d), dev(z), dev(pool_s), dev(pool_d), gf, gw, accumulate=False,
                               row=row.reshape(z.shape).to(torch.int32).to(DEV).contiguous(), presim=presim)
        assert ops.status_poll(True) == 0
        if presim:
            check(form, all_t, grads)
        else:
            assert float(grads.flat.abs().max()) == 0.0            # UFR_GBWD_NO_PRESIM: the volume scatter only
            check(form, all_t, None)
    # accumulate onto non-zero targets (of the gradients' own scale, so that the sum's rounding stays below theirs)
    base = [(torch.rand(t.shape, generator=g) - 0.5) * float(t.abs().max()) for t in gv64]
    all_t = [b.clone().to(DEV) for b in base]
    grads = ops.GradBuffer(DEV)
    ops.project_gather_bwd(fh, weights, grads, dev(o), dev(d), dev(z), dev(sim8), dev(d_pv), all_t[0::2], all_t[1::2], accumulate=True)
    assert ops.status_poll(True) == 0
    check("accumulate", all_t, grads, base=base)


def test_scatter_kept_workspace_with_a_partial_block(weights):
    """The kept-zero workspace form (tests/test_gpu_scatter.py covers NV = 3 with full blocks) at NV = 5 and P % 64 = 8:
    left zero, same gradients, against float64."""
    NV = 5
    fr, fh, o, d, z, d_pv, sim8, gv64, gp64, gv32, gp32, g = _scatter_case(NV, "offaxis", 13, 40, True)
    dev = lambda t: t.to(DEV).contiguous()
    kept = torch.zeros(ops.project_gather_bwd_workspace_floats(fh), device=DEV)
    for it in range(2):
        all_t, gf, gw = _targets(fr, lambda s: torch.full(s, 5.0, device=DEV))
        ops.project_gather_bwd(fh, weights, ops.GradBuffer(DEV), dev(o), dev(d), dev(z), dev(sim8), dev(d_pv), gf, gw,
                               accumulate=False, zeroed_workspace=kept)
        assert ops.status_poll(True) == 0
        assert int(torch.count_nonzero(kept)) == 0
        for a, r32_, r64_ in zip(all_t, gv32, gv64):
            assert _grad_err(a, r64_) < G.bound(_grad_err(r32_, r64_), G.CAP_GRAD), it
