"""The float64 yardsticks of the forward GPU tests (tests/forward_ref.py) are well conditioned on this host.

The GPU bounds of test_gpu_forward_rows.py and test_gpu_compositor_sampler.py widen to twice the float32 oracle's own
distance from float64; that widening must never become the bound.  Here the float32 oracle alone is held under caps that
sit below every GPU bound, on the same seeded inputs (the tokens come from the oracle's gather instead of the HIP one), and
the input recipes are checked to produce the edge cases they claim.
"""
import pytest
import torch

import forward_ref as F

ROW_CAP = 2e-6          # transformers, per row (GPU bound 2e-5; srdf 5e-5)
COMPOSITE_CAP = 1e-5    # compositor forward (GPU bound 5e-6 widened per case) and d_srdf (1e-4)
DRAD_CAP = 1e-5         # d_radiance (1e-5)
DVAR_CAP = 5e-5         # d_variance, relative (1e-4)
SAMPLER_CAP = 5e-6      # importance sampler with the uniform floor (5e-6)


@pytest.mark.parametrize("NV,SN,RN", F.AGG_SHAPES)
def test_float32_oracle_rows_stay_near_float64(NV, SN, RN):
    x, rgbm0, dirs = F.oracle_tokens(NV, RN, SN, seed=NV)
    for masks in F.MASKS:
        rgbm = rgbm0.clone()
        F.force_masks(rgbm, masks)
        none, one = F.mask_census(rgbm)
        if masks == "all_masked":
            assert none >= 1
        if masks == "one_unmasked":
            assert one >= 1
        e = F.errors(F.aggregate_ref(x, rgbm, dirs, RN, SN, torch.float32), F.aggregate_ref(x, rgbm, dirs, RN, SN))
        print(f"MEASURE float32 oracle NV={NV} SN={SN} RN={RN} {masks}: " + "  ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in e.items()))
        for k, (whole, row) in e.items():
            assert whole < ROW_CAP and row < ROW_CAP, (masks, k, whole, row)


@pytest.mark.parametrize("NV", [2, 3, 4, 5, 6, 7])
def test_float32_oracle_view_half_at_any_point_count(NV):
    x, rgbm, dirs = (t[:F.POINTS].clone() for t in F.oracle_tokens(NV, 3, 16, seed=50 + NV))
    none, one = F.alternate_masks(rgbm)
    assert F.mask_census(rgbm)[0] >= len(none) >= 1 and F.mask_census(rgbm)[1] >= len(one) >= 1
    ref = F.view_ref(x, rgbm, dirs)
    assert tuple(ref["token0"].shape) == (F.POINTS, 80) and tuple(ref["radiance"].shape) == (F.POINTS, 3)
    e = F.errors(F.view_ref(x, rgbm, dirs, torch.float32), ref)
    for k, (whole, row) in e.items():
        assert whole < ROW_CAP and row < ROW_CAP, (k, whole, row)
    # points are independent in the reference too: a prefix evaluated alone gives the same rows
    part = F.view_ref(x[:7], rgbm[:7], dirs[:7])
    assert F.row_err(part["token0"], ref["token0"][:7]) < 1e-12 and F.row_err(part["radiance"], ref["radiance"][:7], F.RGB_FLOOR) < 1e-12
    # every view masked: the blend is the plain mean of the views' colours
    mean = rgbm[none, :, :3].double().mean(1)
    assert F.row_err(ref["radiance"][none], mean, F.RGB_FLOOR) < 1e-12


def _composite_check(SN, variance):
    ref, ref32 = F.composite_refs(SN, variance)
    e = F.composite_errors(ref32, ref)
    print(f"MEASURE float32 oracle compositor SN={SN} variance={variance}: {e}")
    for k in F.COMPOSITE_FWD + ("d_srdf",):
        assert e[k] < COMPOSITE_CAP, (k, e[k])
    assert e["d_radiance"] < DRAD_CAP
    if F.dvar_live(ref, ref32):
        assert e["d_variance"] < DVAR_CAP, e["d_variance"]
    else:
        assert abs(ref32["d_variance"]) < F.DVAR_NEGLIGIBLE * ref["dvar_scale"]
    return ref


@pytest.mark.parametrize("SN", F.COMPOSITE_SN)
def test_float32_oracle_compositor_stays_near_float64(SN):
    c = F.composite_inputs(SN)
    assert bool((c["z"][:, 1:] >= c["z"][:, :-1]).all()) and int((c["z"][0, 1:] == c["z"][0, :-1]).sum()) >= 1
    crossings = (c["srdf"][:, 1:] * c["srdf"][:, :-1] < 0)
    down = crossings & (c["srdf"][:, 1:] < 0)
    if SN >= 63:        # surface crossings in both directions
        assert bool(down.any()) and bool((crossings & ~down).any())
    for variance in F.COMPOSITE_VARIANCE:
        ref = _composite_check(SN, variance)
        assert all(bool(torch.isfinite(ref[k]).all()) for k in ("weight", "d_srdf", "d_radiance"))
        if SN >= 63 and variance <= 0.6:
            assert F.dvar_live(*F.composite_refs(SN, variance))
        if variance >= 0.6 and SN >= 17:
            ones = float((F.raw_alpha(c, variance) == 1.0).float().mean())
            assert ones >= 0.2, (variance, ones)        # the inclusive clip passes the gradient at alpha == 1 exactly


@pytest.mark.parametrize("SN", F.COMPOSITE_CLIP_SN)
def test_float32_oracle_compositor_on_the_clips(SN):
    ref = _composite_check(SN, F.CLIP_HIGH)
    assert ref["d_variance"] == 0.0
    # at the low clip pc - nc cancels against the 1e-5 guard: float32 itself is ~1e-2 from float64 there, which is why the GPU
    # test compares that case with the float32 oracle
    lo64, lo32 = F.composite_refs(SN, F.CLIP_LOW)
    assert lo64["d_variance"] == 0.0 and lo32["d_variance"] == 0.0
    e = F.composite_errors(lo32, lo64)
    print(f"MEASURE float32 oracle compositor SN={SN} variance={F.CLIP_LOW}: {e}")
    assert e["weight"] > 1e-4


@pytest.mark.parametrize("SN,PN", F.SAMPLER_SHAPES)
def test_float32_oracle_sampler_stays_near_float64(SN, PN):
    w, z, U2 = F.sampler_inputs(SN, PN)
    assert float(w.min()) >= 0.2 / SN * (1 - 1e-6)        # the uniform floor
    e = F.rel_err(F.sampler_ref(w, z, U2, torch.float32), F.sampler_ref(w, z, U2))
    print(f"MEASURE float32 oracle sampler SN={SN} PN={PN}: {e:.1e}")
    assert e < SAMPLER_CAP
    # the edge patterns, as the reference arithmetic gives them
    for pattern in ("zeros", "onehot_first"):
        w, z, U2 = F.sampler_inputs(SN, PN, pattern)
        assert torch.equal(F.sampler_ref(w, z, U2, torch.float32), z[:, :1].expand(-1, PN)), pattern
    for pattern in F.PATTERNS:
        w, z, U2 = F.sampler_inputs(SN, PN, pattern)
        zf = F.sampler_ref(w, z, U2, torch.float32)
        assert bool(torch.isfinite(zf).all()) and bool((zf >= z[:, :1]).all()) and bool((zf <= z[:, -1:]).all()), pattern
    if SN >= 8:
        z = F.sampler_inputs(SN, PN, "z_ties")[1]
        assert int((z[:, 1:] == z[:, :-1]).sum()) >= 3 * F.SAMPLER_RN
        assert int((F.sampler_inputs(SN, PN, "zero_run")[0] == 0).sum()) >= F.SAMPLER_RN * (SN // 3)


def _check_merge_order(label, v):
    order = F.merge_order(v)
    values, indices = torch.sort(v, dim=-1, stable=True)
    assert torch.equal(order, indices), label
    assert bool(F.same_values(torch.gather(v, -1, order), values).all()), label


def test_merge_order_on_the_edges_of_the_float_order():
    nan, inf = float("nan"), float("inf")
    v = torch.tensor([[nan, 1.0, -0.0, inf, 0.0, nan, -inf, 1.0, 0.0, -0.0, inf, 3e38, -nan, 1.0],
                      [2.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 2.0, 9.0, 9.0, -9.0, 0.0, 1.0, 2.0],
                      [nan] * 14])
    order = F.merge_order(v)
    # a NaN after every number, +inf included; NaNs, equal values and the two zeros in index order
    assert order[0].tolist() == [6, 2, 4, 8, 9, 1, 7, 13, 11, 3, 10, 0, 5, 12]
    assert order[2].tolist() == list(range(14))
    _check_merge_order("edges", v)
    assert bool(F.same_values(v, v).all()) and not bool(F.same_values(v[0, 2], v[0, 4]))      # -0.0 is not +0.0 by bits


@pytest.mark.parametrize("SN,PN", F.SAMPLER_SHAPES)
def test_merge_order_is_the_stable_sort_on_the_poisoned_patterns(SN, PN):
    """The order the GPU tests hold the sampler to (forward_ref.merge_order) is torch.sort(stable=True), the sort of
    model.py:466 and sampler.py:106, on what the poisoned rays put into it: the coarse positions followed by the fine
    samples the float32 reference arithmetic draws from them, the latter in a shuffled order (the reference returns them
    sorted).  The recipes are checked to poison the rays they claim and no other."""
    g = torch.Generator().manual_seed(77 + SN + PN)
    shuffle = torch.randperm(PN, generator=g)
    clean_rays = [r for r in range(F.SAMPLER_RN) if r not in F.POISONED_RAYS]
    assert len(F.POISONS) == len(set(F.POISONS)) == 19
    for poison in F.POISONS:
        (w, z, U2), (wc, zc, Uc) = F.poisoned_sampler_inputs(SN, PN, poison)
        for t, c, dim in ((w, wc, 0), (z, zc, 0), (U2, Uc, 1)):
            assert bool(torch.isfinite(c).all()), poison
            assert torch.equal(t.index_select(dim, torch.tensor(clean_rays)), c.index_select(dim, torch.tensor(clean_rays))), poison
        bad = ~(torch.isfinite(w).all(1) & torch.isfinite(z).all(1) & torch.isfinite(U2).all(0))
        if poison == "w_sum_overflows":
            bad = torch.isinf(w.sum(1))
        assert bad.nonzero().flatten().tolist() == list(F.POISONED_RAYS), poison
        if poison.startswith("unsorted_"):
            assert not bool((zc[:, 1:] >= zc[:, :-1]).all(1).any()), poison       # every ray: the general path
        zf = F.sampler_ref(w, z, U2, torch.float32)[:, shuffle]
        _check_merge_order(f"SN={SN} PN={PN} {poison} fine", zf)
        _check_merge_order(f"SN={SN} PN={PN} {poison} merged", torch.cat([z, zf], 1))
    for pattern in F.PATTERNS:
        w, z, U2 = F.sampler_inputs(SN, PN, pattern)
        _check_merge_order(f"SN={SN} PN={PN} {pattern}", torch.cat([z, F.sampler_ref(w, z, U2, torch.float32)[:, shuffle]], 1))


def test_unsorting_permutation_moves_what_it_may():
    for SN in (2, 3, 16, 255):
        p = F.unsorting_permutation(SN)
        assert sorted(p.tolist()) == list(range(SN)) and p.tolist() != list(range(SN))
    j = F.onehot_mid_index(16)
    p = F.unsorting_permutation(16, keep=(j - 1, j))
    assert p[j] == j and p[j - 1] == j - 1 and p.tolist() != list(range(16))
