"""Restatement of the similarity field (ufr_similarity_field, include/ufr.h) with the oracle's own pieces, in float32 and
float64: ``oracle.ufo_oracle.project`` on grid points, ``pair_similarity`` (A7) of the result, the mean over its 8 groups --
what the reference's ``UFORecon.extract_fields`` computes with ``query_cond_info`` (tests/golden/
make_golden_similarity_field.py runs that and tests/test_similarity_field.py compares).  Beside it the two options of the
kernel: ``n_vis``, the views that see a voxel in front of them and strictly inside the image, and the ``min_views`` rule.

The cases of tests/test_gpu_similarity_field.py live here, so that tests/test_similarity_field.py can prove their stated
properties (voxels behind a camera, outside an image, excluded from a comparison) on the CPU from float64 alone.  CPU only.
"""
from __future__ import annotations

import torch

import gather_ref as G
from oracle import ufo_oracle as O

NVS = (2, 3, 5)                       # 1, 3 and 10 pairs; match_ch 32, 64, 128
# (dim, half width of the cube): no dim a multiple of 64, every z-run shorter than the 64 voxels a wave takes
GRIDS = (((5, 7, 9), 1.0), ((33, 17, 3), 2.5), ((24, 24, 24), 4.0))
# over +-1: grids past one launch tile (64 x 128 x 512 voxels) along x, y and z; a column of the last is eight full runs and
# one of 3 voxels
TILE_GRIDS = ((67, 3, 5), (2, 131, 3), (2, 3, 515))
MAX_EXCLUDED = 0.05                   # share of a grid's voxels with |q.z| < QZ_KEEP in some view
MAX_VIS_EXCLUDED = 0.02               # ... within BORDER_TOL of an image border or with |q.z| < QZ_MIN


def tables(bound_min, bound_max, dim):
    """The reference's coordinate tables (model.py:893-895): torch.linspace in float32 per axis."""
    lo, hi = torch.tensor(bound_min, dtype=torch.float32), torch.tensor(bound_max, dtype=torch.float32)
    return tuple(torch.linspace(lo[a], hi[a], dim[a]) for a in range(3))


def cube_tables(dim, half):
    return tables([-half] * 3, [half] * 3, dim)


def grid_points(tabs):
    """(X Y Z, 3) float32, z fastest: the voxel positions in the order of the field's memory."""
    xx, yy, zz = torch.meshgrid(*tabs, indexing="ij")
    return torch.stack([xx, yy, zz], -1).reshape(-1, 3)


def field_at(frame, pts, dt=torch.float32):
    """The field at ``pts`` (N,3) in dtype ``dt``: u (N,), the projections xy (NV,N,2) and qz (NV,N), n_vis (N,) int64."""
    batch, _, _, match = G.frame_as(frame, dt)
    poses = batch["source_poses"][0]
    NV = poses.shape[0]
    p = pts.to(dt).reshape(-1, 1, 3)
    with torch.no_grad():
        xy, _, _ = O.project(poses, p)
        ph = torch.cat([p, torch.ones_like(p[..., :1])], -1).reshape(-1, 4)
        qz = torch.einsum("vj,pj->vp", poses[:, 2], ph)
        u = O.pair_similarity(xy, match[0][0], NV).mean(-1).reshape(-1)
    xy = xy.reshape(NV, -1, 2)
    seen = (qz > 0) & (xy > -1).all(-1) & (xy < 1).all(-1)
    return dict(u=u, xy=xy, qz=qz, n_vis=seen.sum(0))


def apply_min_views(u, n_vis, min_views):
    """A voxel seen by fewer than ``min_views`` views gets -1.0 exactly."""
    return torch.where(n_vis < min_views, torch.full_like(u, -1.0), u) if min_views > 0 else u


def comparable(r64):
    """(N,) bool: voxels whose similarity is compared -- |q.z| at least QZ_KEEP in every view (the reference is undefined at 0)."""
    return (r64["qz"].abs() >= G.QZ_KEEP).all(0)


def vis_comparable(r64):
    """(N,) bool: voxels whose n_vis is compared -- in every view farther than BORDER_TOL from |x| = 1 and |y| = 1 (an fp32
    evaluation may land on the other side of the strict test) and |q.z| at least QZ_MIN."""
    return ((r64["xy"].abs() - 1.0).abs() > G.BORDER_TOL).all(-1).all(0) & (r64["qz"].abs() >= G.QZ_MIN).all(0)


def shares(r64) -> dict:
    """Shares of a grid's voxels, from float64: behind some camera, outside some image, excluded from either comparison."""
    xy = r64["xy"]
    outside = ((xy <= -1) | (xy >= 1)).any(-1).any(0)
    return dict(behind=float((r64["qz"] <= 0).any(0).double().mean()), outside_image=float(outside.double().mean()),
                excluded=float((~comparable(r64)).double().mean()), vis_excluded=float((~vis_comparable(r64)).double().mean()))
