"""Float64 reference of the gather (ufr_project_gather) and of its volume scatter (ufr_project_gather_bwd), the fp32
yardstick next to it, and seeded ray sets that leave the comfortable geometry of the frame fixtures.

The oracle (oracle/ufo_oracle.py) is dtype-polymorphic: ``rows`` runs ``project``, ``pair_similarity``, ``volume_lookup``
and ``gather_inputs`` on copies of a ``scene.make_frame`` frame and of the weights in the requested dtype -- float64 is
the reference, float32 (the oracle as it stands) the yardstick: a compared quantity's yardstick is the fp32 oracle's own
distance from float64 on the same inputs, and a kernel's bound is ``bound(yardstick, cap)``.  ``scatter_grads`` is autograd
of ``sum(vol24 * d_pv[:, :24]) + sum(pre_sim_mlp(sim8) * d_pv[:, 24:])`` with respect to the six sampled volumes and the
pre_sim_mlp parameters, in either dtype.

Ray sets (``torch.rand`` on a CPU generator only, as in scene.py: identical on every host).  The stepwise entry points
take free ``ray_o``, ``ray_d``, ``z``, so none of them needs a frame of its own:

  offaxis_rays    pixels of the render view; a third of the rays tilted off its axis (they leave the source images), a
                  third started behind the camera arc (their first samples lie behind source cameras), z well beyond
                  near_fars; per-ray origins (stride 3), or one origin for all rays
  cellstep_rays   rays through the centre of source camera v (constant (x, y) in view v) whose samples are exactly one
                  depth cell of stage s apart, plus a fixed fraction: consecutive lanes of the scatter hand a corner over
  repeat_rays     all samples of a ray at one z, at two alternating z, or unsorted

CPU only; tests/test_gather_ref.py proves the stated properties of the sets from the float64 reference alone.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import ufo_oracle as O

STAGES = O.STAGES
PRESIM = "ray_transformer.pre_sim_mlp."
PRESIM_KEYS = tuple(f"{PRESIM}{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias"))
MARGIN = 4.0            # kernel bound = MARGIN x yardstick: v_rcp for a division and fma order are a handful of roundings
CAP_ROWS = 1e-5         # the suite's bound on gathered rows (test_project_gather_rows)
CAP_XY = 5e-6           # ... on projected coordinates
CAP_GRAD = 1e-4         # ... on the scatter's gradients (test_project_gather_bwd_matches_oracle_autograd)
BORDER_TOL = 2e-5       # masks are compared where the float64 projection is farther than this from |x| = 1, |y| = 1 ...
QZ_MIN = 1e-3           # ... and |qz| at least this
QZ_KEEP = 0.05          # the builders keep every sample's |qz| at least this far from 0 (the reference is undefined at 0)
U23 = 2.0 ** -23


def bound(yardstick: float, cap: float) -> float:
    """MARGIN x yardstick, capped by the suite's present bound -- except where the yardstick itself forces more: the
    kernel cannot be asked to be nearer to float64 than twice what the fp32 restatement of the same arithmetic is."""
    return min(MARGIN * yardstick, max(cap, 2.0 * yardstick))


def _cast(x, dt):
    if torch.is_tensor(x):
        return x.to(dt) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: _cast(v, dt) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_cast(v, dt) for v in x]
    return x


def frame_as(frame, dt):
    """(batch, feat, volumes, match) of a scene.Frame in dtype ``dt``."""
    return _cast(frame.batch, dt), _cast(frame.source_imgs_feat, dt), _cast(frame.feature_volume, dt), _cast(frame.match_feature, dt)


def points(ray_o, ray_d, z):
    o = ray_o.reshape(-1, 3)                      # (1,3) broadcast or (RN,3) per ray
    return o[:, None, :] + z[..., None] * ray_d[:, None, :]


def _weight_sum(poses, pts, volumes, near_far):
    """Wsum of volume_lookup (model.py:375-386): the sum over views and stages of the sampled weight volumes."""
    RN, SN, _ = pts.shape
    W = 0
    for n in range(poses.shape[0]):
        _, xyz, _ = O.project(poses[n:n + 1], pts, near_far)
        for st in STAGES:
            W = W + F.grid_sample(volumes[st]["weight_volume"][n:n + 1], xyz.view(1, 1, RN, SN, 3), mode="bilinear",
                                  align_corners=True, padding_mode="zeros")[0, 0, 0]
    return W


def _tap_range(img, xy):
    """Per (view, ray, sample): max - min, and the largest magnitude, of the four texels a bilinear tap
    (align_corners=False, zeros padding) of ``img`` (NV,H,W) reads at ``xy``; a texel outside the image counts as the zero
    it contributes."""
    NV, H, W = img.shape
    ix = ((xy[..., 0] + 1) * W - 1) / 2
    iy = ((xy[..., 1] + 1) * H - 1) / 2
    x0, y0 = torch.floor(ix), torch.floor(iy)
    v = torch.arange(NV).reshape(NV, 1, 1)
    vals = []
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = x0 + dx, y0 + dy
            ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
            t = img[v, cy.clamp(0, H - 1).long(), cx.clamp(0, W - 1).long()]
            vals.append(torch.where(ok, t, torch.zeros_like(t)))
    vals = torch.stack(vals, 0)
    return vals.max(0).values - vals.min(0).values, vals.abs().max(0).values


def rows(P, frame, ray_o, ray_d, z, dt=torch.float64, vol24_in=None, sim8_in=None):
    """Every row-level output of the gather in dtype ``dt``: xy (NV,RN,SN,2), mask_z / inb / mask (NV,RN,SN), qz and the
    frustum depth zn per view, sim8 (RN,SN,8), vol24 (RN,SN,24), wsum (RN,SN), x (P,NV,80), rgb (P,NV,3), dirs (P,NV,3),
    and the depth-PE argument delta = depth tap - z_cam with the two terms (NV,RN,SN).  ``vol24_in`` / ``sim8_in``: the
    form in which RayTransformer.forward receives them."""
    batch, feat, vols, match = frame_as(frame, dt)
    Pd = {k: v.to(dt) for k, v in P.items() if k.startswith(PRESIM)}
    ray_o, ray_d, z = ray_o.to(dt), ray_d.to(dt), z.to(dt)
    RN, SN = z.shape
    pts = points(ray_o, ray_d, z)
    poses = batch["source_poses"][0]
    NV = poses.shape[0]
    s_idx = batch["start_idx"] if "start_idx" in batch else 1
    with torch.no_grad():
        xy, xyz, mask_z = O.project(poses, pts)
        ph = torch.cat([pts, torch.ones_like(pts[..., :1])], -1).reshape(-1, 4)
        qz = torch.einsum("vj,pj->vp", poses[:, 2], ph).reshape(NV, RN, SN)
        nf = batch["near_fars"][0][0]
        zn = ((qz - nf[0]) / (nf[1] - nf[0])) * 2 - 1.0
        out = dict(xy=xy, mask_z=mask_z, qz=qz, zn=zn, pts=pts,
                   pts_err=2.0 ** -24 * ((z[..., None] * ray_d[:, None, :]).abs() + pts.abs()))   # roundings of o + z d in fp32
        if vols is not None and vol24_in is None:
            out["wsum"] = _weight_sum(poses, pts, vols, nf)
        sim8 = O.pair_similarity(xy, match[0][0], NV) if sim8_in is None else sim8_in.to(dt).reshape(RN, SN, 8)
        vol24 = O.volume_lookup(poses, pts, vols, nf) if vol24_in is None else vol24_in.to(dt).reshape(RN, SN, 24)
        x, rgb, dirs, mask = O.gather_inputs(Pd, pts, batch, feat[0], vol24, sim8, xy, mask_z, s_idx)
        inb = ((xy[..., 0] <= 1.) & (xy[..., 0] >= -1.) & (xy[..., 1] <= 1.) & (xy[..., 1] >= -1.)).to(dt)
        depth = batch["depth_info"][0]
        d_s = F.grid_sample(depth[:, None], xy, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
        w2c = batch["w2cs"][0, s_idx:]
        zc = torch.einsum("vj,rsj->vrs", w2c[:, 2, :3], pts) + w2c[:, 2, 3][:, None, None]
        tap_range, tap_max = _tap_range(depth, xy)
        out.update(sim8=sim8, vol24=vol24, x=x, rgb=rgb.permute(2, 3, 0, 1).reshape(RN * SN, NV, 3),
                   dirs=dirs.permute(1, 2, 0, 3).reshape(RN * SN, NV, 3), mask=mask, inb=inb, d_s=d_s, zc=zc, delta=d_s - zc,
                   tap_range=tap_range, tap_max=tap_max)
    return out


def comparable(r64):
    """(NV,RN,SN) bool: the view-samples whose masks are compared -- everything except projections within BORDER_TOL of an
    image border (an fp32 evaluation may land on the other side of the inclusive test) or with |qz| < QZ_MIN."""
    xy = r64["xy"].abs()
    return ((xy - 1.0).abs() > BORDER_TOL).all(-1) & (r64["qz"].abs() >= QZ_MIN)


def geometry_shares(r64) -> dict:
    """Shares of a ray set, from the float64 rows: view-samples behind a camera, outside the image, outside the frustum
    depth, excluded from the mask comparison; points that no view's frustum covers (the blend's weight sum is exactly 0)."""
    return dict(behind=float((r64["qz"] <= 0).double().mean()), outside_image=float((r64["inb"] == 0).double().mean()),
                outside_depth=float((r64["zn"].abs() > 1).double().mean()), excluded=float((~comparable(r64)).double().mean()),
                all_outside=float((r64["wsum"] == 0).double().mean()))


def pe_terms(frame, r32, r64):
    """The three terms (NV,RN,SN,8) of the element-wise bound on |PE - PE64| of the depth encoding sin(2^k pi delta + phase):

      measured   2^k pi |delta32 - delta64|: the propagated argument error of the fp32 restatement
      ulp        an ulp of the argument 2^k pi delta (and of the phase, at most 1)
      forward    2^k pi E, E the first-order forward bound of the roundings on the way to delta, h = 2^-24 per rounding,
                 from float64 quantities only: the point o + z d (2 roundings), a projected coordinate sum_j M_ij p_j +
                 M_i3 (4 roundings, each at most h times the sum of the terms' magnitudes), the division x = qx / qz, the
                 pixel coordinate (2 roundings), the tap (its slope per pixel is at most the range of the four texels it
                 reads: 0 outside the image; 4 roundings of values no larger than the tap's largest texel), z_cam
                 (4 roundings) and the subtraction."""
    h = 2.0 ** -24
    H, W = frame.H, frame.W
    s_idx = frame.batch["start_idx"] if "start_idx" in frame.batch else 1
    M = frame.batch["source_poses"][0].double().abs()                   # (NV,4,4)
    Rz = frame.batch["w2cs"][0, s_idx:, 2].double().abs()               # (NV,4)
    ap, dp = r64["pts"].abs(), r64["pts_err"]                           # (RN,SN,3)
    S = torch.einsum("vij,rsj->virs", M[:, :3, :3], ap) + M[:, :3, 3][:, :, None, None]
    dq = 4 * h * S + torch.einsum("vij,rsj->virs", M[:, :3, :3], dp)    # (NV,3,RN,SN)
    qz = r64["qz"].abs()
    x, y = r64["xy"][..., 0].abs(), r64["xy"][..., 1].abs()
    dx = (dq[:, 0] + x * dq[:, 2]) / qz + h * x
    dy = (dq[:, 1] + y * dq[:, 2]) / qz + h * y
    dix = W / 2 * dx + 2 * h * (W / 2 * (x + 1) + 1)
    diy = H / 2 * dy + 2 * h * (H / 2 * (y + 1) + 1)
    d_tap = r64["tap_range"] * (dix + diy) + 4 * h * r64["tap_max"]
    d_zc = 4 * h * (torch.einsum("vj,rsj->vrs", Rz[:, :3], ap) + Rz[:, 3][:, None, None]) + torch.einsum("vj,rsj->vrs", Rz[:, :3], dp)
    E = d_tap + d_zc + h * (r64["d_s"].abs() + r64["zc"].abs())
    d_delta = (r32["delta"].double() - r64["delta"]).abs()
    freqs = torch.repeat_interleave(math.pi * 2.0 ** torch.arange(0, 4, dtype=torch.float64), 2)
    arg = r64["delta"][..., None] * freqs
    return freqs * d_delta[..., None], U23 * (arg.abs() + 1.0), freqs * E[..., None]


def pe_tolerance(frame, r32, r64):
    """Element-wise bound (NV,RN,SN,8) on |PE - PE64|.  The fp32 restatement is itself ~1e-3 from float64 in the maximum
    norm (delta comes from a bilinear tap of a white-noise depth map: a rounding of the pixel coordinate moves it by
    rounding x the local contrast), so each element is bounded by its own propagated argument error:

        MARGIN x (2^k pi |delta32 - delta64| + an ulp of the argument)  +  2^k pi E

    The first term is the margin times what the fp32 restatement is seen to lose at this element.  That alone is not a bound:
    |delta32 - delta64| is ONE realisation of the roundings on the way to delta and vanishes where they happen to cancel,
    while the kernel's -- an fma where the restatement multiplies and adds -- is another.  So the forward bound E of those
    roundings (pe_terms) is added once, without the margin: to first order no fp32 evaluation of delta, in whatever order
    and with or without fmas, is farther from float64.

    MEASURED on the MI355X over the 60 forward cases: the first term alone is exceeded by the kernel in 20 of them, on 1 to
    18 elements of up to 82 880, by up to 2.54 x (NV 3, 16 x 64) -- elements where delta32 happens to land on delta64 --
    while on most sets the kernel sits at 0.25 = 1 / MARGIN of it, the fp32 restatement's own place.  Against the whole bound
    the kernel's worst element is at 0.155 (NV 3, 27 x 24), the fp32 restatement's at 0.129; no error exceeds 0.32 of the
    forward term alone, so E is pessimistic by about 3 at the worst element."""
    measured, ulp, forward = pe_terms(frame, r32, r64)
    return MARGIN * (measured + ulp) + forward


def scatter_grads(P, frame, ray_o, ray_d, z, sim8, d_pv, dt=torch.float64):
    """Autograd in ``dt`` of sum(vol24 * d_pv[:, :24]) + sum(pre_sim_mlp(sim8) * d_pv[:, 24:]) -> (list of the six dense
    volume gradients in the order feature_volume, weight_volume per stage; dict of the pre_sim_mlp parameter gradients)."""
    batch, _, vols, _ = frame_as(frame, dt)
    vols = {st: {k: v.clone().requires_grad_(True) for k, v in vols[st].items()} for st in STAGES}
    Pd = {k: P[k].to(dt).clone().requires_grad_(True) for k in PRESIM_KEYS}
    pts = points(ray_o.to(dt), ray_d.to(dt), z.to(dt))
    d_pv = d_pv.to(dt)
    vol24 = O.volume_lookup(batch["source_poses"][0], pts, vols, batch["near_fars"][0][0])
    sim16 = O.mlp3(sim8.to(dt).reshape(-1, 8), Pd, PRESIM)
    ((vol24.reshape(-1, 24) * d_pv[:, :24]).sum() + (sim16 * d_pv[:, 24:]).sum()).backward()
    gv = []
    for st in STAGES:
        for k in ("feature_volume", "weight_volume"):
            g = vols[st][k].grad
            gv.append(torch.zeros_like(vols[st][k]) if g is None else g)
    return gv, {k: Pd[k].grad for k in PRESIM_KEYS}


# ----------------------------------------------------------------------------------------------------------- ray sets
def _keep_off_camera_planes(frame, ray_o, ray_d, z):
    """Moves every sample with |qz| < QZ_KEEP in some view along its ray until no view has one (float64 test)."""
    poses = frame.batch["source_poses"][0].double()
    for _ in range(8):
        pts = points(ray_o.double(), ray_d.double(), z.double())
        qz = torch.einsum("vj,rsj->vrs", poses[:, 2, :3], pts) + poses[:, 2, 3][:, None, None]
        bad = (qz.abs() < QZ_KEEP).any(0)
        if not bool(bad.any()):
            return z
        z = torch.where(bad, z + 0.13, z)
    raise AssertionError("could not move the samples off the camera planes")


def _interior_pixels(frame, RN, g):
    """Seeded pixels off the outermost rows and columns: the render view is source view 0 moved along its x axis, so a
    ray through its first or last pixel row projects to |y| = 1 in view 0 at every sample."""
    H, W = frame.H, frame.W
    r = 1 + (torch.rand(RN, generator=g) * (H - 2)).long().clamp_max(H - 3)
    c = 1 + (torch.rand(RN, generator=g) * (W - 2)).long().clamp_max(W - 3)
    return r * W + c


def offaxis_rays(frame, RN, SN, seed, per_ray_origin=True):
    """-> ray_o (RN,3) or (3,), ray_d (RN,3), z (RN,SN).  Ray r is of kind (r + seed) % 3: 0 a pixel ray of the render
    view, 1 the same tilted by up to +-0.175 per component (not renormalised), 2 started from 1.6 x the render origin
    (behind the camera arc) with a quarter of its samples before the camera planes.  z spans (1.7, 4.9) where near_fars is
    about (1.9, 4.2).  With one origin for all rays, that origin is 1.3 x the render origin, kind 2 is a plain pixel ray,
    z spans (2.7, 5.9) and a tenth of every ray's samples lie before the camera planes."""
    g = torch.Generator().manual_seed(1000 + seed)
    idx = _interior_pixels(frame, RN, g)
    d = frame.batch["ray_d"][0][:, idx].t().contiguous()
    kind = (torch.arange(RN) + seed) % 3
    tilt = (torch.rand(RN, 3, generator=g) - 0.5) * 0.35
    d = torch.where((kind == 1)[:, None], d + tilt, d).contiguous()
    o0 = frame.batch["ray_o"][0]
    z = 1.7 + 3.2 * torch.rand(RN, SN, generator=g)
    u, e = torch.rand(RN, SN, generator=g), torch.rand(RN, SN, generator=g)
    if per_ray_origin:
        ray_o = o0[None].repeat(RN, 1)
        ray_o[kind == 2] *= 1.6
        ray_o = ray_o.contiguous()
        z = torch.where((u < 0.25) & (kind == 2)[:, None], 0.3 + 1.4 * e, z)
    else:
        ray_o = (o0 * 1.3).contiguous()
        z = torch.where(u < 0.10, 0.2 + 0.6 * e, z + 1.0)
    z = torch.sort(z, dim=1).values
    return ray_o, d, _keep_off_camera_planes(frame, ray_o, d, z).contiguous()


CELL_FRACTION = 0.37


def cellstep_rays(frame, RN, SN, seed):
    """-> ray_o (RN,3), ray_d (RN,3), z (RN,SN), view (RN,), stage (RN,).  Ray r starts at the centre of source camera
    v = r % NV and aims at a seeded point near the scene centre, so (x, y) is constant in view v; its samples sit at
    frustum depth cells c_j + CELL_FRACTION of stage s = (r // NV) % 3, c_j = j mod (D_s - 1): one cell per lane, wrapping
    to the near plane where the frustum ends (stage 3 has 8 planes)."""
    g = torch.Generator().manual_seed(2000 + seed)
    NV = frame.NV
    cam = frame.batch["source_poses_inv"][0, :, :3, 3].double()
    fwd = frame.batch["w2cs"][0, -NV:, 2, :3].double()          # camera z axes in world coordinates
    nf = frame.batch["near_fars"][0][0].double()
    view = torch.arange(RN) % NV
    stage = (torch.arange(RN) // NV) % 3
    target = (torch.rand(RN, 3, generator=g).double() - 0.5) * 0.6
    d = target - cam[view]
    d = d / d.norm(dim=1, keepdim=True)
    D = torch.tensor([frame.feature_volume[st]["feature_volume"].shape[2] for st in STAGES])[stage]
    j = torch.arange(SN)[None, :]
    cell = (j % (D[:, None] - 1)).double() + CELL_FRACTION
    depth = nf[0] + cell / (D[:, None] - 1).double() * (nf[1] - nf[0])       # camera-z of view v
    z = depth / (d * fwd[view]).sum(1, keepdim=True)
    return cam[view].float().contiguous(), d.float().contiguous(), z.float().contiguous(), view, stage


def shared_corner_share(frame, ray_o, ray_d, z, view, stage) -> float:
    """Share of the consecutive sample pairs (j, j+1) of every ray whose cell in the ray's aligned view and stage steps
    by exactly one along depth with the same (x, y) cell and the shared plane inside the volume -- sample j's far corners
    are then sample j+1's near corners (hand-over (a) of gather_bwd.hip).  From float64 cell indices."""
    poses = frame.batch["source_poses"][0].double()
    nf = frame.batch["near_fars"][0][0].double()
    pts = points(ray_o.double(), ray_d.double(), z.double())
    hits = total = 0
    for r in range(z.shape[0]):
        v, st = int(view[r]), STAGES[int(stage[r])]
        _, xyz, _ = O.project(poses[v:v + 1], pts[r:r + 1], (nf[0], nf[1]))
        D, H, W = frame.feature_volume[st]["feature_volume"].shape[2:]
        c = xyz[0, 0]
        ix, iy, iz = (c[:, 0] + 1) / 2 * (W - 1), (c[:, 1] + 1) / 2 * (H - 1), (c[:, 2] + 1) / 2 * (D - 1)
        fx, fy, fz = torch.floor(ix), torch.floor(iy), torch.floor(iz)
        inside = (fx >= 0) & (fx + 1 <= W - 1) & (fy >= 0) & (fy + 1 <= H - 1)
        share = (fz[1:] == fz[:-1] + 1) & (fx[1:] == fx[:-1]) & (fy[1:] == fy[:-1]) & inside[1:] & (fz[1:] >= 0) & (fz[1:] <= D - 1)
        hits += int(share.sum())
        total += share.numel()
    return hits / max(total, 1)


def repeat_rays(frame, RN, SN, seed):
    """-> ray_o (3,), ray_d (RN,3), z (RN,SN).  Pixel rays of the render view inside the working volume; ray r has all
    samples at one z (r % 3 == 0), at two alternating z (1), or at unsorted z (2)."""
    g = torch.Generator().manual_seed(3000 + seed)
    idx = _interior_pixels(frame, RN, g)
    d = frame.batch["ray_d"][0][:, idx].t().contiguous()
    nf = frame.batch["near_fars"][0][0]
    lo, hi = float(nf[0]) + 0.2, float(nf[1]) - 0.2
    za = lo + (hi - lo) * torch.rand(RN, 1, generator=g)
    zb = lo + (hi - lo) * torch.rand(RN, 1, generator=g)
    zu = lo + (hi - lo) * torch.rand(RN, SN, generator=g)
    kind = (torch.arange(RN) % 3)[:, None]
    even = (torch.arange(SN) % 2 == 0)[None, :]
    z = torch.where(kind == 0, za.expand(RN, SN), torch.where(kind == 1, torch.where(even, za, zb), zu))
    ray_o = frame.batch["ray_o"][0].contiguous()
    return ray_o, d, _keep_off_camera_planes(frame, ray_o, d, z).contiguous()


# ------------------------------------------------------------------------------------------------------------- metrics
def max_over_max(a, b) -> float:
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_floor1(a, b) -> float:
    """max |a - b| / max(|b|, 1) element-wise."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b).abs() / b.abs().clamp_min(1.0)).max())


COLUMN_GROUPS = dict(feat=slice(0, 32), vol=slice(32, 56), sim16=slice(56, 72), pe=slice(72, 80))


def row_errors(got, r64) -> dict:
    """Distances from the float64 rows of one evaluation's xy, sim8, vol24, the feat / vol / sim16 column groups of x, rgb
    and dirs (``got``: the same keys, any float dtype).  The four column groups of x are measured separately: one error over
    all 80 columns lets a small group hide behind a large one."""
    e = dict(xy=rel_floor1(got["xy"], r64["xy"]))
    for k in ("sim8", "vol24", "rgb", "dirs"):
        e[k] = max_over_max(got[k].reshape(r64[k].shape), r64[k])
    for k in ("feat", "vol", "sim16"):
        e[k] = max_over_max(got["x"][..., COLUMN_GROUPS[k]], r64["x"][..., COLUMN_GROUPS[k]])
    return e


ROW_CAPS = dict(xy=CAP_XY, sim8=CAP_ROWS, vol24=CAP_ROWS, rgb=CAP_ROWS, dirs=CAP_ROWS, feat=CAP_ROWS, vol=CAP_ROWS, sim16=CAP_ROWS)


# --------------------------------------------------------------------------------------------------------------- cases
NVS = (2, 3, 4, 5, 6, 7)
# (RN, SN, per-ray origins).  P = RN * SN points in blocks of 64; a grid of fewer than 8 blocks, and the tail blocks of
# one that is not a multiple of 8, skip the block -> XCD remap of gather.hip.
FORWARD_SHAPES = (
    (1, 1, False),      # P = 1
    (1, 40, True),      # P = 40 < 64: one partial block
    (65, 1, True),      # P = 64 + 1, SN = 1: every lane another ray
    (127, 1, False),    # P = 64 + 63
    (3, 24, True),      # P = 64 + 8
    (8, 64, False),     # 8 blocks exactly
    (13, 40, True),     # P = 520: 8 + 1 blocks, the tail block partial
    (27, 24, True),     # P = 648: 8 + 3 blocks, partial
    (37, 40, False),    # P = 1480: 24 = 3 x 8 blocks, the last (remapped) one partial
    (16, 64, True),     # 16 full blocks
)
POOL_SHAPE = (37, 40, True)     # the view count's largest set: its yardstick also serves the smaller shapes (see yardstick)
STATS_MIN_POINTS = 256          # the shares of a ray set are asserted on the shapes with at least this many points
# the scatter: (ray set, RN, SN, per-ray origins) per view count -- the forward grid thinned
BACKWARD_CASES = (
    ("offaxis", 13, 40, True),      # P % 64 = 8
    ("offaxis", 65, 1, True),       # SN = 1
    ("offaxis", 27, 24, False),     # SN not a multiple of 16, one origin
    ("cellstep", 0, 24, True),      # RN = 3 NV rays: every (view, stage) once
    ("cellstep", 0, 16, True),
    ("repeat", 9, 40, False),       # P % 64 = 40
)


def frame_for(NV):
    from uforecon_amd.scene import make_frame

    return make_frame(48, 64, NV, seed=60 + NV, train_layout=(NV % 2 == 0))     # both layouts: s_idx = 0 and 1


SUPPLIED_SHAPES = ("rays", "aggregate")


def supplied_rays(frame, shape):
    """The sets of the vol24_in / sim8_in form.  'rays': 5 x 40 off-axis samples.  'aggregate': the shape autograd.Aggregate
    calls -- SN = 1, the 7 x 11 points of an off-axis set as per-ray origins, zero directions, z = 1."""
    if shape == "rays":
        return offaxis_rays(frame, 5, 40, frame.NV + 10, True)
    o0, d0, z0 = offaxis_rays(frame, 7, 11, frame.NV + 20, True)
    o = points(o0, d0, z0).reshape(-1, 3).contiguous()
    return o, torch.zeros_like(o), torch.ones(o.shape[0], 1)


def backward_rays(frame, kind, RN, SN, per_ray, seed):
    if kind == "offaxis":
        return offaxis_rays(frame, RN, SN, seed, per_ray)
    if kind == "cellstep":
        return cellstep_rays(frame, 3 * frame.NV, SN, seed)[:3]
    return repeat_rays(frame, RN, SN, seed)


def yardstick(case: dict, pool: dict) -> dict:
    """Per quantity: the larger of the case's own fp32-vs-float64 distance and that of the view count's POOL_SHAPE set
    (same frame, same builder).  A distance is a sample maximum: over the 8 similarities of a single point it
    underestimates what the same arithmetic reaches over 1 480 points, and the kernel's error at that point is another draw
    from the same distribution."""
    return {k: max(case[k], pool[k]) for k in case}
