"""The ray path on rays that are not finite: the sampler's slot -> row table stays whole, a NaN stays in its own ray.

The importance sampler writes, per ray, a table that names the pool row of every merged slot; the ray transformer, the
compositor and their adjoints index the sample pool through it without a range check.  The table is whole only if the
sampler's ranks are a permutation, and they are one only if NaNs have a place in its order.  The order is stated in
tests/forward_ref.py (merge_order: torch.sort(stable=True), pinned without a GPU by tests/test_forward_refs.py), the
poisoned rays are forward_ref.POISONS, applied to rays 1, 4 and 8 of a batch of 9 whose other rays keep finite inputs:
a poisoned and a clean ray share a workgroup.

The sampler tests prefill every output with a sentinel (ops.sample_importance_pool allocates with torch.empty, where stale
contents can stand in for a slot that was never written) and run the sampler kernel alone: it indexes with clamped search
results and with ranks below SN + PN whatever its inputs hold.  The consumer tests hand the table to the kernels that index
with it; the whole-path tests render rays whose index lies outside the image.
"""
import pytest
import torch

import forward_ref as F
from helpers import CASES, case_inputs, load_weights
from uforecon_amd import _lib, ops
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7777.0          # finite, and held by no input: positions lie in [2, 4], weights in [0, 1] or at 3e38
CLEAN_RAYS = [r for r in range(F.SAMPLER_RN) if r not in F.POISONED_RAYS]
OUTPUTS = ("z_fine", "z_all", "z_all_pool", "z_new", "row")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype != torch.float32 else t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ the sampler alone
def _launch(w, z, U2):
    """ufr_sample_importance_merge and ufr_sample_importance_pool into outputs prefilled with SENTINEL / -1"""
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    RN, SN = z.shape
    PN = U2.shape[0]
    wd, zd, ud = w.to(DEV).contiguous(), z.to(DEV).contiguous(), U2.to(DEV).contiguous()
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)      # noqa: E731
    z_fine, z_all, z_all_pool, z_new = full(RN, PN), full(RN, SN + PN), full(RN, SN + PN), full(RN, PN)
    row = torch.full((RN, SN + PN), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.ufr_sample_importance_merge(wd.data_ptr(), zd.data_ptr(), ud.data_ptr(), z_fine.data_ptr(), z_all.data_ptr(),
                                               RN, SN, PN, stream), "ufr_sample_importance_merge")
    _lib.check(lib.ufr_sample_importance_pool(wd.data_ptr(), zd.data_ptr(), ud.data_ptr(), z_all_pool.data_ptr(), z_new.data_ptr(),
                                              row.data_ptr(), RN, SN, PN, stream), "ufr_sample_importance_pool")
    torch.cuda.synchronize()
    return dict(z_fine=z_fine.cpu(), z_all=z_all.cpu(), z_all_pool=z_all_pool.cpu(), z_new=z_new.cpu(), row=row.cpu())


def _holes(r) -> dict:
    """slots nobody wrote, per output"""
    return {k: int((r[k] == (-1 if k == "row" else SENTINEL)).sum()) for k in OUTPUTS}


def _pool_rows(RN, SN, PN) -> torch.Tensor:
    """(RN, SN+PN): the pool rows of every ray in the order of the concatenation [coarse | new]"""
    ray = torch.arange(RN)[:, None]
    return torch.cat([ray * SN + torch.arange(SN), RN * SN + ray * PN + torch.arange(PN)], 1)


def _table_properties(label, z, r):
    """What must hold on EVERY ray whatever it carries: z (RN,SN) the coarse positions as given to the kernel"""
    RN, SN = z.shape
    PN = r["z_new"].shape[1]
    assert not any(_holes(r).values()), (label, _holes(r))
    rows, row = _pool_rows(RN, SN, PN), r["row"].long()
    assert torch.equal(torch.sort(row, dim=1)[0], rows), label                         # a permutation of the ray's own rows
    merged = torch.cat([z, r["z_new"]], 1)
    order = F.merge_order(merged)
    assert bool(F.same_values(r["z_all"], torch.gather(merged, 1, order)).all()), label      # the multiset, in the stated order
    assert torch.equal(row, torch.gather(rows, 1, order)), label                       # ... ties and NaNs in index order
    pool = torch.cat([z.reshape(-1), r["z_new"].reshape(-1)])
    assert bool(F.same_values(pool[row], r["z_all"]).all()), label
    assert torch.equal(F.merge_order(r["z_new"]), torch.arange(PN).expand(RN, PN)), label    # z_new stands in the stated order
    assert bool(F.same_values(r["z_new"], r["z_fine"]).all()), label
    assert bool(F.same_values(r["z_all_pool"], r["z_all"]).all()), label


@pytest.mark.parametrize("SN,PN", F.SAMPLER_SHAPES)
def test_sampler_tables_stay_whole_on_poisoned_rays(SN, PN):
    """Every slot of every output is written, the table of every ray is a permutation of that ray's SN coarse and PN new
    rows in the stated order, the clean rays come out bit for bit as in a launch of the all-clean batch, and two launches
    agree.  The kernel this test was written against ranked with `o < v || (o == v && j < k)` alone, where every NaN gets
    rank 0 among its peers: on that kernel, on an MI355X, the test failed at all twelve shapes, at SN = PN = 16 with
    16 / 8 / 31 / 1 .. 4 unwritten slots of 32 per poisoned ray for one NaN weight / one +inf weight / every position NaN /
    one NaN position (at 256 + 256: 256 / 128 / 511 / 1 .. 4 of 512), and 15 of the 16 slots of z_fine for any of the weight
    patterns; on the kernel that counts a NaN's rank it passes with no slot unwritten."""
    launched = {}
    for poison in F.POISONS:
        (w, z, U2), clean = F.poisoned_sampler_inputs(SN, PN, poison)
        launched[poison] = (z, _launch(w, z, U2), _launch(w, z, U2), _launch(*clean))
    holes = {p: _holes(r) for p, (z, r, again, c) in launched.items()}
    print(f"MEASURE sampler SN={SN} PN={PN}, unwritten slots over the {len(F.POISONED_RAYS)} poisoned rays (row of {SN + PN} each): "
          + "  ".join(f"{p} {h['row']}" for p, h in holes.items())
          + "; z_fine: " + "  ".join(f"{p} {h['z_fine']}" for p, h in holes.items()))
    for poison, (z, r, again, c) in launched.items():
        label = f"SN={SN} PN={PN} {poison}"
        _table_properties(label, z, r)
        for k in OUTPUTS:
            assert torch.equal(_bits(r[k]), _bits(again[k])), (label, k)
            assert torch.equal(_bits(r[k][CLEAN_RAYS]), _bits(c[k][CLEAN_RAYS])), (label, k)
    # the all-clean batches themselves (sorted, and permuted: the general path) meet the same properties
    for poison in ("w_nan_first", "unsorted_z_nan_first"):
        _table_properties(f"SN={SN} PN={PN} clean batch of {poison}", F.poisoned_sampler_inputs(SN, PN, poison)[1][1], launched[poison][3])


# ------------------------------------------------------------------ the kernels that index with the table
@pytest.fixture(scope="module")
def weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


def _consume_status():
    """whatever a NaN cotangent left in the sticky status is reported here, not in the next test"""
    try:
        ops.status_poll(True)
    except UfrError:
        pass
    assert ops.status_poll(True) == 0


def _through_the_table(weights, pool_tok, pool_rad, tab, RN, S2, transformer: bool, base, d_rgb, d_depth):
    """The pool form of every consumer (reads and writes through ``row``) beside the materialised-slot form"""
    row, z = tab["row"].to(DEV).contiguous(), tab["z_all_pool"].to(DEV).contiguous()
    rows = row.reshape(-1).long()
    var = weights.variance.reshape(1)
    out = {}
    if transformer:
        out["srdf"] = ops.ray_transform(weights, pool_tok, RN, S2, row=row)
        out["srdf_slots"] = ops.ray_transform(weights, pool_tok[rows].contiguous(), RN, S2)
        srdf = out["srdf"]
    else:
        srdf = torch.sin(torch.arange(RN * S2, device=DEV, dtype=torch.float32)).view(RN, S2) * 0.2
    out["composite"] = ops.composite(z, pool_rad, srdf, var, row=row)
    out["composite_slots"] = ops.composite(z, pool_rad[rows].view(RN, S2, 3).contiguous(), srdf, var)
    acc = base.clone()
    _, out["d_srdf"], _ = ops.composite_bwd(z, pool_rad, srdf, var, d_rgb, d_depth, None, None, row=row, d_radiance=acc, accumulate=True)
    d_rad_s, out["d_srdf_slots"], _ = ops.composite_bwd(z, pool_rad[rows].view(RN, S2, 3).contiguous(), srdf, var, d_rgb, d_depth, None, None)
    out["d_radiance"], out["d_radiance_slots"] = acc, base.clone()
    out["d_radiance_slots"][rows] += d_rad_s.view(-1, 3)
    if transformer:
        ga, gb = ops.GradBuffer(DEV), ops.GradBuffer(DEV)
        pa, pb = torch.zeros_like(pool_tok), torch.zeros_like(pool_tok)
        ops.ray_transform_bwd(weights, ga, pool_tok, RN, S2, out["d_srdf"], row=row, out=(pa, pb))
        sa, sb = ops.ray_transform_bwd(weights, gb, pool_tok[rows].contiguous(), RN, S2, out["d_srdf_slots"])
        out["d_token0"], out["d_token0_slots"] = (pa, pb), (sa, sb)
    torch.cuda.synchronize()
    _consume_status()
    return out, rows.cpu()


@pytest.mark.parametrize("SN,PN", [(32, 32), (17, 5)])
def test_consumers_read_and_write_inside_the_ray(SN, PN, weights):
    """The tables of the poisoned batches, as the sampler writes them, in ufr_ray_transform, ufr_composite and their
    adjoints over a FINITE random pool (the positions z_all keep their NaNs): the pool form equals the materialised-slot
    form on every ray, and the clean rays equal the all-clean batch bit for bit -- forwards, and in the rows the adjoints
    write.  Gradients of weights and of the variance are not compared: they are sums over all rays, which a NaN
    legitimately reaches.  SN + PN = 22 is no multiple of 16: ufr_ray_transform refuses it (asserted), the compositor and
    its adjoint run."""
    RN, S2, P1 = F.SAMPLER_RN, SN + PN, F.SAMPLER_RN * SN
    transformer = S2 % 16 == 0
    g = torch.Generator().manual_seed(5 + SN)
    pool_tok = torch.randn(RN * S2, 80, generator=g).to(DEV)
    pool_rad = torch.rand(RN * S2, 3, generator=g).to(DEV)
    base = torch.randn(RN * S2, 3, generator=g).to(DEV)
    d_rgb, d_depth = torch.randn(RN, 3, generator=g).to(DEV), torch.randn(RN, generator=g).to(DEV)
    if not transformer:
        with pytest.raises(UfrError, match="multiple of 16"):
            ops.ray_transform(weights, pool_tok, RN, S2, row=torch.zeros(RN, S2, dtype=torch.int32, device=DEV))
    clean_rows = torch.cat([_pool_rows(RN, SN, PN)[r] for r in CLEAN_RAYS])
    same = lambda a, b: bool(F.same_values(a.cpu(), b.cpu()).all())       # noqa: E731
    clean_out = {}
    for poison in F.POISONS:
        label = f"SN={SN} PN={PN} {poison}"
        (w, z, U2), clean = F.poisoned_sampler_inputs(SN, PN, poison)
        tab, tab_clean = _launch(w, z, U2), _launch(*clean)
        _table_properties(label, z, tab)                # the producer's guarantee, before anything indexes with the table
        _table_properties(label + " (clean batch)", clean[1], tab_clean)
        kind = poison.startswith("unsorted_")
        if kind not in clean_out:
            clean_out[kind] = _through_the_table(weights, pool_tok, pool_rad, tab_clean, RN, S2, transformer, base, d_rgb, d_depth)[0]
        a, rows = _through_the_table(weights, pool_tok, pool_rad, tab, RN, S2, transformer, base, d_rgb, d_depth)
        c = clean_out[kind]
        # the pool form against the materialised slots, on every ray (NaN where the ray's positions are NaN, in both)
        if transformer:
            assert torch.equal(a["srdf"], a["srdf_slots"]) and bool(torch.isfinite(a["srdf"]).all()), label
            assert torch.equal(a["srdf"][CLEAN_RAYS], c["srdf"][CLEAN_RAYS]), label
        for x, y, cx in zip(a["composite"], a["composite_slots"], c["composite"]):
            assert same(x, y), label
            assert bool(torch.isfinite(x[CLEAN_RAYS]).all()) and torch.equal(x[CLEAN_RAYS], cx[CLEAN_RAYS]), label
        # the adjoints, held on the clean rays to the comparisons of test_pool_rows_in_the_kernels_equal_materialised_slots
        assert torch.equal(a["d_srdf"][CLEAN_RAYS], a["d_srdf_slots"][CLEAN_RAYS]), label
        assert torch.equal(a["d_srdf"][CLEAN_RAYS], c["d_srdf"][CLEAN_RAYS]), label
        got, want = a["d_radiance"].cpu()[clean_rows], a["d_radiance_slots"].cpu()[clean_rows]
        assert bool(torch.isfinite(got).all()) and torch.allclose(got, want, rtol=0, atol=1e-6), label
        assert torch.equal(got, c["d_radiance"].cpu()[clean_rows]), label
        if transformer:
            inv = torch.empty_like(rows)
            inv[rows] = torch.arange(rows.numel())                       # pool row -> slot
            for p, s, cp in zip(a["d_token0"], a["d_token0_slots"], c["d_token0"]):
                p, s, cp = p.cpu(), s.cpu(), cp.cpu()
                assert bool(torch.isfinite(p[clean_rows]).all()) and torch.equal(p[clean_rows], s[inv[clean_rows]]), label
                assert torch.equal(p[clean_rows], cp[clean_rows]), label
    assert ops.status_poll(True) == 0


# ------------------------------------------------------------------ the whole path on ray indices outside the image
BAD_AT = (5, 18, 36)        # of 37 rays: two share their 4-ray workgroups with clean rays, the last one stands alone in its own


def _outside_indices(name):
    fr, idx, U1, U2, g = case_inputs(name)
    H, W = CASES[name]["H"], CASES[name]["W"]
    assert fr.batch["ray_d"][0].shape[-1] == H * W
    n = 37
    good = idx[:, :n].clone()
    assert bool(((good >= 0) & (good < H * W)).all())
    bad = good.clone()
    for at, v in zip(BAD_AT, (-1, H * W, 2 ** 40)):
        bad[0, at] = v
    return fr, good.contiguous(), bad.contiguous(), U1[:, :n].contiguous(), U2[:, :n].contiguous()


def _render_outside(name, precision, coarse_only):
    fr, good, bad, U1, U2 = _outside_indices(name)
    f = fr.to(DEV)
    fh = ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)
    W = ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()}, precision=precision)
    u2 = None if coarse_only else U2.to(DEV)
    assert ops.status_poll(True) == 0
    want = ops.render_rays(fh, W, good.to(DEV), U1.to(DEV), u2, coarse_only=coarse_only)
    assert ops.status_poll(True) == 0
    got = ops.render_rays(fh, W, bad.to(DEV), U1.to(DEV), u2, coarse_only=coarse_only)
    torch.cuda.synchronize()
    # the non-finite report, then a clean poll: nothing leaks into the next test
    with pytest.raises(UfrError, match="NaN among"):
        ops.status_poll(True)
    assert ops.status_poll(True) == 0
    keep = [r for r in range(good.numel()) if r not in BAD_AT]
    assert bool(got["depth"][list(BAD_AT)].isnan().all()) and bool(got["rgb"][list(BAD_AT)].isnan().all())
    for k in ("depth", "depth_z", "rgb", "srdf", "z_all"):
        assert bool(torch.isfinite(want[k]).all()), k
        assert torch.equal(got[k][keep], want[k][keep]), k
    assert bool(got["z_all"][list(BAD_AT)].isnan().all())


@pytest.mark.parametrize("precision", [ops.PRECISION_FP32, ops.PRECISION_16BIT], ids=["fp32", "16bit"])
def test_ray_indices_outside_the_image_render_nan_and_nothing_else(precision):
    """ufr_render_rays, coarse and fine pass, with the indices -1, H*W and 2^40 among 37 rays: ray_setup_kernel gives those
    rays NaN near / far, every position of both passes is NaN, the sampler still hands the fine pass a whole table, depth and
    colour of the three come out NaN, and every other ray is bit for bit what it is beside valid neighbours."""
    _render_outside("c2_hier_small", precision, coarse_only=False)


def test_ray_indices_outside_the_image_coarse_only():
    """The same on the coarse-only configuration, which involves no table: the promise of ray_setup_kernel's comment"""
    _render_outside("c1_coarse_only", ops.PRECISION_FP32, coarse_only=True)
