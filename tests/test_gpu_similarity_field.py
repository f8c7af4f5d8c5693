"""The similarity-field kernel (ufr_similarity_field, csrc/similarity_field.hip) against the float64 restatement of
tests/similarity_field_ref.py, at 1, 3 and 10 view pairs, on grids that leave the images and pass behind the cameras
(tests/test_similarity_field.py proves those shares on the CPU).

Bound: the project's rule for gathered rows, ``gather_ref.bound(yardstick, CAP_ROWS)``; the yardstick is the float32
restatement's own distance from float64 on the same voxels, computed here on the CPU -- never taken from the kernel.  Only
voxels with |q.z| < QZ_KEEP in some view (float64) are left out of the similarity comparison, at most 5 % of a grid; n_vis is
compared exactly outside BORDER_TOL of an image border and |q.z| < QZ_MIN, at most 2 % left out."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gather_ref as G
import mcubes_ref
import similarity_field_ref as S
from helpers import load_weights
from uforecon_amd import _lib, ops
from uforecon_amd import similarity_field as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(NV, gi) for NV in S.NVS for gi in range(len(S.GRIDS))]


@functools.lru_cache(maxsize=None)
def _frame(NV):
    fr = G.frame_for(NV)
    f = fr.to(DEV)
    return fr, ops.FrameHandle(f.batch, f.source_imgs_feat, f.feature_volume, f.match_feature)


@functools.lru_cache(maxsize=None)
def _reference(NV, dim, half):
    """(r32, r64) of a cube grid, computed once and shared."""
    fr, _ = _frame(NV)
    pts = S.grid_points(S.cube_tables(dim, half))
    return S.field_at(fr, pts, torch.float32), S.field_at(fr, pts, torch.float64)


def _field(NV, dim, half, **kw):
    _, fh = _frame(NV)
    out = ops.similarity_field(fh, [-half] * 3, [half] * 3, dim, **kw)
    assert ops.status_poll(True) == 0
    return out


def _check_u(tag, u, r32, r64, keep):
    """u (N,) on the host against float64 on the voxels ``keep``, within bound(yardstick, CAP_ROWS)."""
    yard = float((r32["u"].double() - r64["u"])[keep].abs().max())
    err = float((u.double() - r64["u"])[keep].abs().max())
    tol = G.bound(yard, G.CAP_ROWS)
    print(f"{tag}: err {err:.3e} yardstick {yard:.3e} bound {tol:.3e} compared {int(keep.sum())}/{keep.numel()}")
    assert torch.isfinite(u).all(), tag
    assert err <= tol, (tag, err, yard, tol)


@pytest.mark.parametrize("NV,gi", CASES)
def test_field_and_visibility_match_float64(NV, gi):
    dim, half = S.GRIDS[gi]
    r32, r64 = _reference(NV, dim, half)
    u, n_vis = _field(NV, dim, half, return_visibility=True)
    assert tuple(u.shape) == dim and u.dtype == torch.float32 and tuple(n_vis.shape) == dim and n_vis.dtype == torch.uint8
    keep = S.comparable(r64)
    assert float((~keep).double().mean()) <= S.MAX_EXCLUDED
    _check_u(f"NV={NV} {dim}", u.cpu().reshape(-1), r32, r64, keep)
    vkeep = S.vis_comparable(r64)
    assert float((~vkeep).double().mean()) <= S.MAX_VIS_EXCLUDED
    nv = n_vis.cpu().reshape(-1).long()
    assert int(nv.max()) <= NV                                   # every voxel written (the buffer starts at 255)
    assert torch.equal(nv[vkeep], r64["n_vis"][vkeep])
    # the visibility output changes nothing about the field
    assert torch.equal(_field(NV, dim, half), u)


@pytest.mark.parametrize("NV,gi", CASES)
def test_min_views_masks_exactly_and_leaves_the_rest(NV, gi):
    dim, half = S.GRIDS[gi]
    u0 = _field(NV, dim, half)
    u1, n_vis = _field(NV, dim, half, min_views=NV, return_visibility=True)
    fails = n_vis < NV
    if half > 1.0:
        assert bool(fails.any()) and bool((~fails).any())
    assert bool((u1[fails] == -1.0).all())
    assert torch.equal(u1[~fails], u0[~fails])                   # bit-identical (finite values: no NaN to trip the comparison)
    _, r64 = _reference(NV, dim, half)
    vkeep = S.vis_comparable(r64)
    want = S.apply_min_views(r64["u"], r64["n_vis"], NV)
    assert torch.equal((u1.cpu().reshape(-1) == -1.0)[vkeep], (want == -1.0)[vkeep])


@pytest.fixture(scope="module")
def weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


@pytest.mark.parametrize("NV,gi", CASES)
def test_the_gathers_sim8_gives_the_same_field(weights, NV, gi):
    """An independent kernel: ufr_project_gather on the same points -- columns as rays along z, ray_d = (0, 0, 1), z = the z
    table -- and the mean of its sim8 over the 8 columns, within the same bound of float64."""
    dim, half = S.GRIDS[gi]
    r32, r64 = _reference(NV, dim, half)
    _, fh = _frame(NV)
    gx, gy, gz = S.cube_tables(dim, half)
    xx, yy = torch.meshgrid(gx, gy, indexing="ij")
    o = torch.stack([xx, yy, torch.zeros_like(xx)], -1).reshape(-1, 3).contiguous()
    d = torch.tensor([0., 0., 1.]).expand(o.shape[0], 3).contiguous()
    z = gz[None].expand(o.shape[0], -1).contiguous()
    _, _, _, dbg = ops.project_gather(fh, weights, o.to(DEV), d.to(DEV), z.to(DEV), want_sim8=True)
    assert ops.status_poll(True) == 0
    keep = S.comparable(r64)
    _check_u(f"gather NV={NV} {dim}", dbg["sim8"].cpu().mean(-1).reshape(-1), r32, r64, keep)


@pytest.mark.parametrize("NV", S.NVS)
def test_field_mesh_equals_the_restatement_on_the_kernels_field(NV):
    """`field_mesh` at level 0.1 on the 24^3 grid: non-empty, and exactly marching cubes (tests/mcubes_ref.py) of the
    downloaded GPU field mapped to the scene -- the same volume, so no threshold crossing can differ."""
    dim, half = S.GRIDS[2]
    u = _field(NV, dim, half)
    verts, faces, normals = SF.field_mesh(u, [-half] * 3, [half] * 3, level=0.1)
    assert len(verts) > 0 and len(faces) > 0
    v, f, n = mcubes_ref.marching_cubes((-u).cpu().numpy(), ops.marching_cubes_table(), -0.1)
    steps = torch.tensor([d - 1 for d in dim], dtype=torch.float32)
    want = torch.from_numpy(v) / steps * (2 * half) + (-half)
    assert np.array_equal(faces.cpu().numpy(), f) and np.array_equal(normals.cpu().numpy(), n)
    assert torch.equal(verts.cpu(), want)


@pytest.mark.parametrize("NV", S.NVS)
def test_rerun_is_bit_identical_and_a_64_cube_matches(NV):
    dim, half = S.GRIDS[2]
    assert torch.equal(_field(NV, dim, half), _field(NV, dim, half))
    dim, half = (64, 64, 64), 1.5
    u = _field(NV, dim, half)
    assert not bool(torch.isnan(u).any())
    fr, _ = _frame(NV)
    idx = torch.randperm(64 ** 3, generator=torch.Generator().manual_seed(NV))[:4096]
    pts = S.grid_points(S.cube_tables(dim, half))[idx]
    r32, r64 = S.field_at(fr, pts, torch.float32), S.field_at(fr, pts, torch.float64)
    keep = S.comparable(r64)
    assert float((~keep).double().mean()) <= S.MAX_EXCLUDED
    _check_u(f"NV={NV} 64^3 subset", u.cpu().reshape(-1)[idx], r32, r64, keep)


@pytest.mark.parametrize("dim", S.TILE_GRIDS)
def test_grids_beyond_one_launch_tile_and_runs_longer_than_a_wave(dim):
    """The coordinate tables travel as kernel arguments, a tile of 64 x 128 x 512 voxels per launch: grids that cross a tile
    border along x, y and z (the last one also has columns of several 64-voxel runs and a partial one)."""
    NV, half = 3, 1.0
    r32, r64 = _reference(NV, dim, half)
    u, n_vis = _field(NV, dim, half, return_visibility=True)
    keep = S.comparable(r64)
    assert bool(keep.all())
    _check_u(f"tiles {dim}", u.cpu().reshape(-1), r32, r64, keep)
    vkeep = S.vis_comparable(r64)
    assert torch.equal(n_vis.cpu().reshape(-1).long()[vkeep], r64["n_vis"][vkeep])


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    _, fh = _frame(3)
    tabs = [torch.linspace(-1, 1, 8) for _ in range(3)]
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    u = torch.full((8, 8, 8), float("nan"), device=DEV)
    call = lambda frame, dim, out, mv: lib.ufr_similarity_field(frame, fp(tabs[0]), fp(tabs[1]), fp(tabs[2]), (C.c_int32 * 3)(*dim),  # noqa: E731
                                                                out, None, mv, None)
    ok = C.byref(fh.frame)
    assert call(None, (8, 8, 8), u.data_ptr(), 0) == -1 and b"ufr_similarity_field" in lib.ufr_last_error()
    assert call(C.byref(_lib.Frame()), (8, 8, 8), u.data_ptr(), 0) == -1                  # a handle that was never prepared
    assert call(ok, (8, 8, 8), None, 0) == -1 and b"null" in lib.ufr_last_error()
    assert call(ok, (8, 1, 8), u.data_ptr(), 0) == -1 and b"8x1x8" in lib.ufr_last_error()
    assert call(ok, (2048, 1024, 1024), u.data_ptr(), 0) == -1 and b"2^31" in lib.ufr_last_error()
    assert call(ok, (8, 8, 8), u.data_ptr(), -1) == -1 and b"min_views" in lib.ufr_last_error()
    assert call(ok, (8, 8, 8), u.data_ptr(), 4) == -1 and b"min_views" in lib.ufr_last_error()
    assert ops.status_poll(True) == 0
    assert bool(torch.isnan(u).all())                                                      # nothing was launched
    with pytest.raises(ops.UfrError):
        ops.similarity_field(fh, [-1] * 3, [1] * 3, (8, 1, 8))
    assert call(ok, (8, 8, 8), u.data_ptr(), 3) == 0 and ops.status_poll(True) == 0 and not bool(torch.isnan(u).any())


def _pipeline_args():
    return argparse.Namespace(extract_geometry=True, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64,
                              fine_sample=64, volume_type="correlation", volume_reso=96, mvs_depth_guide=1,
                              depth_pos_encoding=True, use_dir_srdf=False, explicit_similarity=True,
                              test_coarse_only=False, test_ray_num=800, test_n_view=3, out_dir=None)


def test_extract_similarity_end_to_end(tmp_path, capsys):
    """Images -> encoder -> field -> mesh file, on the small synthetic batch of tests/test_pipeline.py."""
    from uforecon_amd import pipeline
    from uforecon_amd.scene import fill_state_dict, make_frame

    H, W, NV = 32, 64, 3
    batch = make_frame(H, W, NV, seed=0).to(DEV).batch
    pm = {}
    for st, s in (("stage1", 4), ("stage2", 2), ("stage3", 1)):
        p = torch.zeros(1, NV, 2, 4, 4, device=DEV)
        p[0, :, 0] = batch["w2cs"][0, :NV]
        K = batch["intrinsics"][0, :NV].clone()
        K[:, :2] = K[:, :2] / s
        p[0, :, 1, :3, :3] = K
        p[0, :, 1, 3, 3] = 1.0
        pm[st] = p
    batch["proj_matrices"] = pm
    near, far = float(batch["near_fars"][0, 0, 0]), float(batch["near_fars"][0, 0, 1])
    batch["depth_values_org_scale"] = torch.linspace(near, far, 48, device=DEV)[None]
    batch["meta"] = ["dtu-scan24-3-00000000"]
    net = fill_state_dict(pipeline.UFOReconInference(_pipeline_args()), 21).eval().to(DEV)
    net.load_state_dict(load_weights(), strict=False)
    handles = []
    inner = net.frame_handle
    net.frame_handle = lambda *a, **k: handles.append(inner(*a, **k)) or handles[-1]
    u = net.extract_similarity(batch, resolution=16)
    assert u.is_cuda and tuple(u.shape) == (16, 16, 16) and bool(torch.isfinite(u).all())
    assert torch.equal(u, ops.similarity_field(handles[-1], [-1.] * 3, [1.] * 3, 16))
    assert "fraction occupied" in capsys.readouterr().out
    assert not list(tmp_path.iterdir())                          # no out_dir, no file
    level = float(u.median())
    u2 = net.extract_similarity(batch, resolution=16, threshold=level, out_dir=str(tmp_path))
    assert torch.equal(u2, ops.similarity_field(handles[-1], [-1.] * 3, [1.] * 3, 16))
    lines = open(tmp_path / "sim_scan24_16.ply").read().split("\n")
    assert lines[0] == "ply"
    V = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    F = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    body = lines[lines.index("end_header") + 1:]
    assert V > 0 and F > 0 and len([ln for ln in body if ln]) == V + F
    verts = np.array([[float(t) for t in ln.split()[:3]] for ln in body[:V]])
    assert verts.min() >= -1.0 and verts.max() <= 1.0            # scene coordinates of the +-1 cube, not voxel indices
    faces = np.array([[int(t) for t in ln.split()] for ln in body[V:V + F]])
    assert (faces[:, 0] == 3).all() and faces[:, 1:].min() >= 0 and faces[:, 1:].max() < V
