"""The stated properties of the gather tests' ray sets (tests/gather_ref.py), proven from the float64 reference alone
(CPU only): how much of each off-axis set lies behind a camera, outside the images, outside the frustum depth and outside
every frustum; how little is excluded from the exact mask comparison; that the cell-step sets do step one cell per sample."""
import pytest
import torch

import gather_ref as G
from helpers import load_weights


def _every_offaxis_set(fr):
    """Every set the GPU module compares masks on: the forward matrix, the scatter's off-axis cases, the supplied form."""
    NV = fr.NV
    shapes = list(G.FORWARD_SHAPES) + [(RN, SN, per_ray) for kind, RN, SN, per_ray in G.BACKWARD_CASES if kind == "offaxis"]
    for RN, SN, per_ray in dict.fromkeys(shapes):
        o, d, z = G.offaxis_rays(fr, RN, SN, NV, per_ray)
        assert tuple(o.shape) == ((RN, 3) if per_ray else (3,)) and tuple(d.shape) == (RN, 3) and tuple(z.shape) == (RN, SN)
        yield (RN, SN, per_ray), o, d, z
    for shape in G.SUPPLIED_SHAPES:
        yield shape, *G.supplied_rays(fr, shape)


@pytest.mark.parametrize("NV", G.NVS)
def test_offaxis_sets_leave_the_comfortable_geometry(NV):
    fr = G.frame_for(NV)
    P = load_weights()
    for name, o, d, z in _every_offaxis_set(fr):
        r64 = G.rows(P, fr, o, d, z)
        r32 = G.rows(P, fr, o, d, z, torch.float32)
        s = G.geometry_shares(r64)
        print(NV, name, {k: round(v, 3) for k, v in s.items()})
        assert float(r64["qz"].abs().min()) >= G.QZ_KEEP                  # |qz| kept away from 0 by construction
        # masks are compared exactly on everything but these; nothing else is ever excluded
        assert s["excluded"] <= 0.02
        cmp = G.comparable(r64)
        assert torch.equal(r32["mask"].double()[cmp], r64["mask"][cmp])   # the fp32 oracle agrees wherever masks are compared
        assert torch.equal(r32["mask_z"].double()[cmp], r64["mask_z"][cmp])
        if z.numel() < G.STATS_MIN_POINTS:
            continue
        assert s["behind"] >= 0.02
        assert s["outside_image"] >= 0.20
        assert s["outside_depth"] >= 0.20
        assert 0.05 <= s["all_outside"] <= 0.40     # beyond that too little of the volume path is exercised


@pytest.mark.parametrize("NV", G.NVS)
def test_cellstep_sets_share_corners(NV):
    fr = G.frame_for(NV)
    for SN in (16, 24):
        o, d, z, view, stage = G.cellstep_rays(fr, 3 * NV, SN, NV)
        assert sorted(set(zip(view.tolist(), stage.tolist()))) == [(v, s) for v in range(NV) for s in range(3)]
        assert G.shared_corner_share(fr, o, d, z, view, stage) >= 0.5
        r64 = G.rows(load_weights(), fr, o, d, z)
        # (x, y) of a ray is constant in its aligned view: the ray passes through that camera's centre
        for r in range(z.shape[0]):
            xy = r64["xy"][int(view[r]), r]
            assert float((xy - xy[:1]).abs().max()) < 1e-5
        assert float(r64["qz"].abs().min()) >= G.QZ_KEEP


@pytest.mark.parametrize("NV", (2, 5))
def test_repeat_sets_repeat(NV):
    fr = G.frame_for(NV)
    o, d, z = G.repeat_rays(fr, 9, 40, NV)
    assert float((z[0] - z[0, 0]).abs().max()) == 0.0                       # one z
    assert torch.equal(z[1, 0::2], z[1, :1].expand(20)) and torch.equal(z[1, 1::2], z[1, 1:2].expand(20)) and z[1, 0] != z[1, 1]
    assert not bool((z[2, 1:] >= z[2, :-1]).all())                          # unsorted
    r64 = G.rows(load_weights(), fr, o, d, z)
    assert float((r64["wsum"] > 0).double().mean()) > 0.9                   # inside the working volume


def test_scatter_reference_matches_finite_differences():
    """The float64 scatter reference is the adjoint of the lookup: <d vol24, J dV> = <J^T d vol24, dV> for a random dV."""
    from oracle import ufo_oracle as O

    NV = 3
    fr = G.frame_for(NV)
    P = load_weights()
    o, d, z = G.offaxis_rays(fr, 13, 40, NV, True)
    g = torch.Generator().manual_seed(5)
    d_pv = torch.rand(13 * 40, 40, generator=g) - 0.5
    sim8 = torch.rand(13 * 40, 8, generator=g) * 2 - 1
    gv, gp = G.scatter_grads(P, fr, o, d, z, sim8, d_pv)
    batch, _, vols, _ = G.frame_as(fr, torch.float64)
    pts = G.points(o.double(), d.double(), z.double())
    f = lambda V: (O.volume_lookup(batch["source_poses"][0], pts, V, batch["near_fars"][0][0]).reshape(-1, 24) * d_pv[:, :24].double()).sum()
    dV = {st: {k: torch.rand(v.shape, generator=g).double() - 0.5 for k, v in vols[st].items()} for st in G.STAGES}
    h = 1e-6
    Vp = {st: {k: vols[st][k] + h * dV[st][k] for k in vols[st]} for st in G.STAGES}
    Vm = {st: {k: vols[st][k] - h * dV[st][k] for k in vols[st]} for st in G.STAGES}
    fd = float(f(Vp) - f(Vm)) / (2 * h)
    an = sum(float((gv[2 * i + j] * dV[st][k]).sum()) for i, st in enumerate(G.STAGES) for j, k in enumerate(("feature_volume", "weight_volume")))
    assert abs(fd - an) < 1e-6 * max(abs(an), 1.0), (fd, an)
    assert all(float(v.abs().max()) > 0 for v in gp.values())
