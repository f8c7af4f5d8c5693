"""The compositor (forward and adjoint) and the importance sampler with its merge against the oracle in float64.

Inputs and references: tests/forward_ref.py (tests/test_forward_refs.py keeps them well conditioned on any host).  Each
bound is the project's existing one, at least twice the float32 oracle's own distance from float64 on the same case.

Compositor: every lane-ownership class of SN in [2, 256] x inv_s from 1 to 8103, where up to half the samples have a raw
alpha of exactly 1.0 (the inclusive clip passes the gradient there), and inv_s on both ends of its [1e-6, 1e6] clip, where
d_variance is exactly zero.  Sampler: exact properties of the merge (sortedness, bit-identity with torch.sort, the row table
a permutation) on every shape and weight pattern -- all-zero, one-hot, flat CDF stretches, equal coarse positions, unsorted
coarse positions (the general rank path) -- and the fine positions against float64.
"""
import pytest
import torch

import forward_ref as F
from helpers import rel_err
from uforecon_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------ compositor
def _composite(SN, variance):
    c = {k: v.to(DEV) for k, v in F.composite_inputs(SN).items()}
    var = torch.tensor([variance], dtype=torch.float32, device=DEV)
    rgb, depth, opacity, weight = ops.composite(c["z"], c["radiance"], c["srdf"], var)
    d_rad, d_srdf, d_var = ops.composite_bwd(c["z"], c["radiance"], c["srdf"], var, c["d_rgb"], c["d_depth"], c["d_opacity"],
                                             c["d_weight"])
    out = dict(weight=weight, rgb=rgb, depth=depth, opacity=opacity, d_radiance=d_rad, d_srdf=d_srdf)
    out = {k: v.cpu() for k, v in out.items()}
    out["d_variance"] = float(d_var)
    return out


def _fmt(e):
    return "  ".join(f"{k} {'-' if v is None else format(v, '.1e')}" for k, v in e.items())


def _check_composite(label, got, ref64, ref32, keys):
    e, y = F.composite_errors(got, ref64), F.composite_errors(ref32, ref64)
    print(f"MEASURE {label}: {_fmt(e)}   (float32 oracle: {_fmt(y)})   d_variance {got['d_variance']:.6e} "
          f"(float64 {ref64['d_variance']:.6e}, float32 resolution scale {ref64['dvar_scale']:.1e}, "
          f"{'relative' if F.dvar_live(ref64, ref32) else 'absolute'} check)")
    for k in keys:
        assert bool(torch.isfinite(got[k]).all()), (label, k)
        assert e[k] < F.bound(F.COMPOSITE_BOUNDS[k], y[k]), (label, k, e[k], y[k])
    return e, y


@pytest.mark.parametrize("variance", F.COMPOSITE_VARIANCE)
@pytest.mark.parametrize("SN", F.COMPOSITE_SN)
def test_composite_and_adjoint_against_float64(SN, variance):
    ref64, ref32 = F.composite_refs(SN, variance)
    got = _composite(SN, variance)
    e, y = _check_composite(f"compositor SN={SN} variance={variance}", got, ref64, ref32, F.COMPOSITE_FWD + ("d_radiance", "d_srdf"))
    if F.dvar_live(ref64, ref32):
        assert e["d_variance"] < F.bound(F.COMPOSITE_BOUNDS["d_variance"], y["d_variance"]), (e["d_variance"], y["d_variance"])
    else:
        # the true value is cancellation or underflow (forward_ref.dvar_live): nothing to be relative to
        assert abs(got["d_variance"]) < F.DVAR_NEGLIGIBLE * ref64["dvar_scale"], (got["d_variance"], ref64["dvar_scale"])


@pytest.mark.parametrize("SN", F.COMPOSITE_CLIP_SN)
def test_composite_with_inv_s_on_its_upper_clip(SN):
    """variance 1.5: exp(15) clips to 1e6.  torch's clip passes no gradient outside its range (the kernel's s_live gate):
    d_variance is exactly zero; the forward and d_srdf meet the same bounds as inside the range."""
    ref64, ref32 = F.composite_refs(SN, F.CLIP_HIGH)
    got = _composite(SN, F.CLIP_HIGH)
    _check_composite(f"compositor SN={SN} variance={F.CLIP_HIGH}", got, ref64, ref32, F.COMPOSITE_FWD + ("d_radiance", "d_srdf"))
    assert ref64["d_variance"] == 0.0 and got["d_variance"] == 0.0


# one ulp of a float32 sigmoid at 0.5 (2^-24) against the 1e-5 guard, in each of the two sigmoids
LOW_CLIP_BOUND = 2 * 2.0 ** -24 / 1e-5


@pytest.mark.parametrize("SN", F.COMPOSITE_CLIP_SN)
def test_composite_with_inv_s_on_its_lower_clip(SN):
    """variance -1.5: exp(-15) clips to 1e-6.  d_variance is exactly zero and everything stays finite.  The forward is
    compared with the FLOAT32 oracle: with inv_s = 1e-6 both sigmoids sit within 1e-8 of 0.5, so pc - nc is a difference of
    a few float32 ulps next to the 1e-5 guard, and the float32 reference itself is 6e-3 .. 8e-3 from float64 -- no float64
    bound means anything here.  Two float32 evaluations of the same formula may still differ by one ulp of either sigmoid
    (the exponential is another implementation): LOW_CLIP_BOUND."""
    ref64, ref32 = F.composite_refs(SN, F.CLIP_LOW)
    got = _composite(SN, F.CLIP_LOW)
    e32 = {k: rel_err(got[k], ref32[k]) for k in F.COMPOSITE_FWD}
    print(f"MEASURE compositor SN={SN} variance={F.CLIP_LOW} against the float32 oracle: {_fmt(e32)}   "
          f"(float32 oracle against float64: {_fmt(F.composite_errors(ref32, ref64))})")
    assert ref32["d_variance"] == 0.0 and got["d_variance"] == 0.0
    for k in ("weight", "rgb", "depth", "opacity", "d_radiance", "d_srdf"):
        assert bool(torch.isfinite(got[k]).all()), k
    for k, v in e32.items():
        assert v < LOW_CLIP_BOUND, (k, v)


# ------------------------------------------------------------------ importance sampler and merge
def _sample(w, z, U2):
    wd, zd, ud = w.to(DEV).contiguous(), z.to(DEV).contiguous(), U2.to(DEV).contiguous()
    z_fine, z_all = ops.sample_importance_merge(wd, zd, ud)
    z_all_pool, z_new, row = ops.sample_importance_pool(wd, zd, ud)
    return dict(z_fine=z_fine.cpu(), z_all=z_all.cpu(), z_all_pool=z_all_pool.cpu(), z_new=z_new.cpu(), row=row.cpu().long())


def _exact_properties(label, z, r):
    """What must hold bit for bit whatever the weights: z (RN,SN) the coarse positions as given to the kernel"""
    RN, SN = z.shape
    PN = r["z_fine"].shape[1]
    assert tuple(r["z_all"].shape) == (RN, SN + PN) and tuple(r["row"].shape) == (RN, SN + PN), label
    assert bool((r["z_all"][:, 1:] >= r["z_all"][:, :-1]).all()), label
    assert torch.equal(r["z_fine"], torch.sort(r["z_fine"], dim=1)[0]), label
    assert torch.equal(r["z_new"], r["z_fine"]), label
    assert torch.equal(r["z_all"], torch.sort(torch.cat([z, r["z_fine"]], 1), dim=1)[0]), label
    assert torch.equal(r["z_all_pool"], r["z_all"]), label
    ray = torch.arange(RN)[:, None]
    rows = torch.cat([ray * SN + torch.arange(SN), RN * SN + ray * PN + torch.arange(PN)], 1)      # ascending per ray
    assert torch.equal(torch.sort(r["row"], dim=1)[0], rows), label
    pool = torch.cat([z.reshape(-1), r["z_new"].reshape(-1)])
    assert torch.equal(pool[r["row"]], r["z_all"]), label


@pytest.mark.parametrize("SN,PN", F.SAMPLER_SHAPES)
def test_importance_sampler_and_merge_properties_and_positions(SN, PN):
    RN = F.SAMPLER_RN
    # positions against float64, on weights whose CDF steps all stay away from zero
    w, z, U2 = F.sampler_inputs(SN, PN)
    r = _sample(w, z, U2)
    _exact_properties(f"SN={SN} PN={PN} bump", z, r)
    ref64, ref32 = F.sampler_ref(w, z, U2), F.sampler_ref(w, z, U2, torch.float32)
    e, y = rel_err(r["z_fine"], ref64), rel_err(ref32, ref64)
    e_all = rel_err(r["z_all"], torch.sort(torch.cat([z.double(), ref64], 1), dim=1)[0])
    assert e < F.bound(F.SAMPLER_BOUND, y) and e_all < F.bound(F.SAMPLER_BOUND, y), (e, e_all, y)

    # the edges, compared with what the reference arithmetic gives for them
    edge = {}
    for pattern in F.PATTERNS[1:]:
        w, z, U2 = F.sampler_inputs(SN, PN, pattern)
        r = _sample(w, z, U2)
        _exact_properties(f"SN={SN} PN={PN} {pattern}", z, r)
        if pattern in ("zeros", "onehot_first"):
            # a CDF without a step: every fine sample is the first coarse position
            assert torch.equal(r["z_fine"], z[:, :1].expand(RN, PN)), pattern
            # ... and the stable merge keeps the coarse sample in front of its PN copies
            assert torch.equal(r["row"][:, 0], torch.arange(RN) * SN), pattern
            assert torch.equal(r["row"][:, 1:PN + 1], RN * SN + torch.arange(RN)[:, None] * PN + torch.arange(PN)), pattern
        else:
            edge[pattern] = rel_err(r["z_fine"], F.sampler_ref(w, z, U2, torch.float32))
            assert edge[pattern] < F.SAMPLER_BOUND, (pattern, edge[pattern])

    # unsorted coarse positions: the general rank path
    w, z, U2 = F.sampler_inputs(SN, PN)
    perm = F.unsorting_permutation(SN)
    zp = z[:, perm].contiguous()
    assert not bool((zp[:, 1:] >= zp[:, :-1]).all())
    r = _sample(w[:, perm].contiguous(), zp, U2)
    _exact_properties(f"SN={SN} PN={PN} unsorted", zp, r)
    # ... against the sorted-input path where the two are comparable: a one-hot weight whose slot and left neighbour stay in
    # place gives the same CDF and the same bracketing positions, hence the same fine samples; the merge then sees the
    # same multiset of coarse positions in another order
    comparable = SN >= 4
    if comparable:
        j = F.onehot_mid_index(SN)
        w, z, U2 = F.sampler_inputs(SN, PN, "onehot_mid")
        perm = F.unsorting_permutation(SN, keep=(j - 1, j))
        zp = z[:, perm].contiguous()
        assert not bool((zp[:, 1:] >= zp[:, :-1]).all())
        a, b = _sample(w, z, U2), _sample(w[:, perm].contiguous(), zp, U2)
        _exact_properties(f"SN={SN} PN={PN} unsorted one-hot", zp, b)
        for k in ("z_fine", "z_new", "z_all"):
            assert torch.equal(a[k], b[k]), k
    print(f"MEASURE sampler SN={SN} PN={PN}: z_fine {e:.1e} z_all {e_all:.1e} of float64 (float32 oracle {y:.1e}); edge patterns "
          f"against the float32 oracle: " + "  ".join(f"{k} {v:.1e}" for k, v in edge.items())
          + f"; unsorted: exact properties hold{', merge equals the sorted-input one' if comparable else ''}")
