"""The similarity field on the CPU: the oracle restatement (tests/similarity_field_ref.py) against the reference's own
`extract_fields` (tests/golden/similarity_field_small.npz), the coordinate tables, `field_mesh`'s coordinate map, and the
stated properties of the grids tests/test_gpu_similarity_field.py runs -- proved from float64 alone."""
import os

import numpy as np
import pytest
import torch

import gather_ref as G
import mcubes_ref
import similarity_field_ref as S
from uforecon_amd import ops
from uforecon_amd import similarity_field as SF

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "similarity_field_small.npz"))


@pytest.mark.parametrize("NV", S.NVS)
def test_restatement_equals_the_references_extract_fields(golden, NV):
    """float32, resolution 9 over +-1 and +-4: the field IS pair_similarity (A7) of the projected grid points, to the bit, at
    every view count (measured: a maximum absolute difference of 0.0 at NV = 2, 3 and 5)."""
    fr = G.frame_for(NV)
    for half in (1, 4):
        want = golden[f"u/nv{NV}/b{half}"]
        got = S.field_at(fr, S.grid_points(S.cube_tables((9, 9, 9), float(half))))["u"].reshape(9, 9, 9).numpy()
        assert want.shape == (9, 9, 9) and np.isfinite(want).all()
        assert np.array_equal(got, want), (NV, half, float(np.abs(got - want).max()))


@pytest.mark.parametrize("lo,hi,res", [((-1., -1., -1.), (1., 1., 1.), 9), ((-2.5, -0.1, 0.3), (2.5, 0.7, 4.0), (33, 17, 3)),
                                       ((-4., -4., -4.), (4., 4., 4.), (24, 24, 24))])
def test_coordinate_tables_equal_torch_linspace(lo, hi, res):
    """What the kernel is handed = the reference's torch.linspace per axis in float32 (model.py:893-895), bit for bit, also
    where a bound is no float32 number."""
    dim = (res,) * 3 if isinstance(res, int) else res
    tabs = ops.grid_tables(lo, hi, res)
    b0, b1 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    for a in range(3):
        want = torch.linspace(b0[a], b1[a], dim[a])
        assert tabs[a].dtype == torch.float32 and tabs[a].is_contiguous() and not tabs[a].is_cuda
        assert torch.equal(tabs[a], want)
        assert torch.equal(S.tables(lo, hi, dim)[a], want)
    with pytest.raises(ops.UfrError):
        ops.grid_tables(lo, hi, (4, 4))


def test_field_mesh_maps_voxels_to_the_scene_and_winds_like_a_tsdf(monkeypatch):
    """A ball of high similarity in a 17x13x21 grid over an off-centre box: `field_mesh` = marching cubes of (-u, -level)
    (run here through the numpy restatement of the kernel) mapped by v / (dim - 1) (max - min) + min.  The vertices lie on the
    ball in SCENE coordinates, the normals and the faces' winding point out of the occupied region."""
    table = ops.marching_cubes_table()
    seen = {}

    def on_host(vol, level=0.0):
        seen["vol"], seen["level"] = vol.clone(), level
        v, f, n = mcubes_ref.marching_cubes(vol.numpy(), table, level)
        return torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n)

    monkeypatch.setattr(ops, "marching_cubes", on_host)
    lo, hi, dim = (-1.0, 0.5, 2.0), (3.0, 2.5, 8.0), (17, 13, 21)
    centre, radius = torch.tensor([1.2, 1.4, 5.1]), 0.7
    pts = S.grid_points(S.tables(lo, hi, dim)).reshape(*dim, 3)
    u = 0.9 - (pts - centre).norm(dim=-1) + radius      # u = 0.9 on the sphere
    verts, faces, normals = SF.field_mesh(u, lo, hi, level=0.9)
    assert torch.equal(seen["vol"], -u) and seen["level"] == -0.9
    assert len(verts) > 100 and len(faces) > 100
    # scene coordinates: on the sphere up to the linear interpolation of the distance inside a cell, h^2 / (8 r) = 0.016 for
    # the longest cell edge h = 0.3
    assert float(((verts - centre).norm(dim=-1) - radius).abs().max()) < 0.025
    # ... and exactly the stated map of the voxel-index vertices
    v_idx = torch.from_numpy(mcubes_ref.marching_cubes((-u).numpy(), table, -0.9)[0])
    steps = torch.tensor([d - 1 for d in dim], dtype=torch.float32)
    assert torch.equal(verts, v_idx / steps * (torch.tensor(hi) - torch.tensor(lo)) + torch.tensor(lo))
    out = torch.nn.functional.normalize(verts - centre, dim=-1)
    # the normals are gradients in voxel-index space: anisotropic cells tilt them, they still point outwards
    assert float((normals * out).sum(-1).min()) > 0.5
    tri = verts[faces.long()]
    face_n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
    outward = (face_n * (tri.mean(1) - centre)).sum(-1)       # a vertex exactly on a grid point leaves a few zero-area faces
    assert bool((outward > -1e-6).all()) and float((outward > 0).float().mean()) > 0.95
    assert SF.resolution_tag(512) == "512" and SF.resolution_tag((64, 64, 64)) == "64" and SF.resolution_tag((5, 7, 9)) == "5x7x9"


@pytest.mark.parametrize("NV", S.NVS)
def test_gpu_grids_leave_the_comfortable_geometry(NV):
    """From float64 alone, for the grids of tests/test_gpu_similarity_field.py: the share of voxels excluded from the
    similarity comparison (|q.z| < QZ_KEEP in some view) stays under 5 %, from the visibility comparison under 2 %; the
    +-4 cube has at least 15 % of its voxels behind some camera and 80 % outside some image, the +-2.5 slab 60 % outside; no
    dim is a multiple of 64 and every z-run is shorter than a wave's 64 voxels (TILE_GRIDS and the 64^3 grid cover the rest)."""
    fr = G.frame_for(NV)
    for dim, half in S.GRIDS:
        sh = S.shares(S.field_at(fr, S.grid_points(S.cube_tables(dim, half)), torch.float64))
        assert sh["excluded"] <= S.MAX_EXCLUDED and sh["vis_excluded"] <= S.MAX_VIS_EXCLUDED, (dim, sh)
        assert all(d % 64 for d in dim) and dim[2] < 64
        if half == 4.0:
            assert sh["behind"] >= 0.15 and sh["outside_image"] >= 0.8, sh
        if half == 2.5:
            assert sh["outside_image"] >= 0.6, sh
    if NV == 3:     # the view count the tile grids run at: nothing of them is excluded
        for dim in S.TILE_GRIDS:
            r64 = S.field_at(fr, S.grid_points(S.cube_tables(dim, 1.0)), torch.float64)
            assert bool(S.comparable(r64).all()) and S.shares(r64)["vis_excluded"] <= S.MAX_VIS_EXCLUDED
    assert [d > t for d, t in zip((S.TILE_GRIDS[0][0], S.TILE_GRIDS[1][1], S.TILE_GRIDS[2][2]), (64, 128, 512))] == [True] * 3


def test_min_views_rule_and_visibility_restatement():
    """n_vis counts the views with q.z > 0 and the projection STRICTLY inside the image; min_views = NV leaves the voxels all
    views see and sets the rest to -1.0 exactly."""
    fr = G.frame_for(3)
    r = S.field_at(fr, S.grid_points(S.cube_tables((24, 24, 24), 4.0)), torch.float64)
    assert int(r["n_vis"].min()) == 0 and int(r["n_vis"].max()) == 3
    masked = S.apply_min_views(r["u"], r["n_vis"], 3)
    assert torch.equal(masked[r["n_vis"] == 3], r["u"][r["n_vis"] == 3]) and bool((masked[r["n_vis"] < 3] == -1.0).all())
    assert S.apply_min_views(r["u"], r["n_vis"], 0) is r["u"]


def test_command_refusals_are_extract_geometrys(tmp_path, capsys):
    """A flag value the mirror does not implement ends the command with one line and exit code 2, before any device work."""
    base = ["--test_dir", str(tmp_path), "--out_dir", str(tmp_path / "o"), "--depth_pos_encoding", "--mvs_depth_guide", "1", "--explicit_similarity"]
    for extra, word in ((["--volume_type", "featuregrid"], "volume_type"), (["--use_dir_srdf"], "use_dir_srdf"),
                        (["--resolution", "1"], "resolution"), (["--min_views", "4"], "min_views")):
        with pytest.raises(SystemExit) as e:
            SF.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
