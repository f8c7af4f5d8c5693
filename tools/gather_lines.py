"""CPU line model of gather_kernel: distinct 128-byte cache lines per 64-lane load instruction, by block shape.

The gather's limit is the L1's line rate, and how many lines one load instruction touches depends on
which 64 points share a wave.  For the benchmark's scene (scene.make_frame(512, 640, 3, seed=0), row-major pixel rays in
chunks of 4096, seeded uniforms) this projects the coarse samples and two stand-ins for the fine ones with the oracle's
formulas, rebuilds the byte address of every tap of phase A (colour, depth guide, the three frustums) and of the
cooperative 32-channel gathers (image features, both sides of every view pair), and counts distinct lines per
instruction under

  1x64   64 consecutive samples of one ray (one 64-sample ray per block)
  RxS    R x-adjacent rays x S consecutive samples, ray index fastest in the lane number: 4x16, 8x8, 16x4

and, for the cooperative phase (one instruction = 8 footprints x 8 lanes of 4 channels), under the two item orders
"point-major" (item = point * NV + view: an instruction mixes views) and "view-major" (8 consecutive local points of
one view).  Fine stand-ins: `surface` draws the importance samples from a Gaussian weight profile (sigma 2 bins) around
a plane at the middle of the depth range, i.e. neighbouring pixels see the same surface; `flat` draws them from
constant weights, i.e. independent uniform positions per ray (what random-init weights give: the pessimistic end).

    python tools/gather_lines.py [--chunks 3] [--markdown]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ufo_oracle as O  # noqa: E402
from uforecon_amd.scene import make_frame, sampler_uniforms  # noqa: E402

LINE = 128
SHAPES = ((1, 64), (4, 16), (8, 8), (16, 4))
VOL_REC = 48                       # bytes per voxel record: 8 features + weight + 3 pad floats


def distinct(lines: np.ndarray) -> float:
    """lines (..., L) int64, -1 = masked lane (reads no line): mean distinct non-negative values over the last axis."""
    a = np.sort(lines, axis=-1)
    new = np.concatenate([a[..., :1] >= 0, (a[..., 1:] != a[..., :-1]) & (a[..., 1:] >= 0)], -1)
    return float(new.sum(-1).mean())


def waves(a: np.ndarray, R: int, S: int) -> np.ndarray:
    """(RN, SN, ...) -> (blocks, 64, ...), local point = sample_in_block * R + ray_in_block (ray fastest)."""
    RN, SN = a.shape[:2]
    a = a.reshape(RN // R, R, SN // S, S, *a.shape[2:])
    a = np.moveaxis(a, (0, 2, 3, 1), (0, 1, 2, 3))
    return a.reshape(-1, R * S, *a.shape[4:])


def taps2d(x, y, W, H, align_corners, border):
    """-> texel index (4, ...) int64 with -1 for a masked corner (zeros padding)."""
    if align_corners:
        ix, iy = (x + 1) / 2 * (W - 1), (y + 1) / 2 * (H - 1)
    else:
        ix, iy = ((x + 1) * W - 1) / 2, ((y + 1) * H - 1) / 2
    if border:
        ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = x0 + dx, y0 + dy
            if border:
                cx, cy = np.clip(cx, 0, W - 1), np.clip(cy, 0, H - 1)
            ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
            out.append(np.where(ok, cy * W + cx, -1).astype(np.int64))
    return np.stack(out)


def taps3d(x, y, zn, W, H, D):
    ix, iy, iz = (x + 1) / 2 * (W - 1), (y + 1) / 2 * (H - 1), (zn + 1) / 2 * (D - 1)
    x0, y0, z0 = np.floor(ix), np.floor(iy), np.floor(iz)
    out = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cx, cy, cz = x0 + dx, y0 + dy, z0 + dz
                ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & (cz >= 0) & (cz <= D - 1)
                out.append(np.where(ok, (cz * H + cy) * W + cx, -1).astype(np.int64))
    return np.stack(out)


def to_lines(texel, rec_bytes, offset=0):
    return np.where(texel >= 0, (texel * rec_bytes + offset) // LINE, -1)


def phase_a(fr, xy, zn):
    """{load family: (RN, SN, NV, n_instr) line ids}: every load instruction of phase A and the frustum phase, per lane
    (a wave is one view, so the view axis stays separate)."""
    H, W = fr.H, fr.W
    x, y = xy[..., 0], xy[..., 1]                            # (NV, RN, SN)
    fam = {}
    t = taps2d(x, y, W, H, False, False)                     # (4, NV, RN, SN)
    fam["colour (16 B texel)"] = to_lines(t, 16)
    fam["depth guide (4 B texel)"] = to_lines(t, 4)
    for st in O.STAGES:
        D, h, w = fr.feature_volume[st]["feature_volume"].shape[2:]
        t3 = taps3d(x, y, zn, w, h, D)                       # (8, NV, RN, SN)
        fam[f"frustum {st} ({D}x{h}x{w})"] = np.concatenate([to_lines(t3, VOL_REC, o) for o in (0, 16, 32)])
    return {k: np.moveaxis(v, (0, 1), (3, 2)) for k, v in fam.items()}       # (RN, SN, NV, n_instr)


def coop(fr, xy, NV):
    """Texel line ids of the cooperative gathers per (RN, SN, item-of-point, corner): image features (one item per view)
    and the two sides of the pair similarities (one item per pair; each side is a load instruction of its own)."""
    h, w = fr.H // 4, fr.W // 4
    x, y = xy[..., 0], xy[..., 1]
    tf = taps2d(x, y, w, h, False, False)                    # (4, NV, RN, SN): 128-byte texels, a line each
    feat = np.where(tf >= 0, tf + np.arange(NV)[None, :, None, None] * h * w, -1)
    tm = taps2d(x, y, w, h, True, True)
    mline = (NV - 1) * 32 * 4 // LINE                        # lines per matching texel
    side_a, side_b = [], []
    for a in range(NV - 1):
        for b in range(a, NV - 1):                           # pair (a, b): (view a, chunk b) against (view b + 1, chunk a)
            side_a.append((a * h * w + tm[:, a]) * mline + b)
            side_b.append(((b + 1) * h * w + tm[:, b + 1]) * mline + a)
    mv = lambda t: np.moveaxis(t, (0, 1), (3, 2))
    return mv(feat), mv(np.stack(side_a, 1)), mv(np.stack(side_b, 1))


def coop_lines(a, R, S, view_major):
    """a (RN, SN, K, 4): K items per point.  One instruction = 8 consecutive items of the block's order."""
    b = waves(a, R, S)                                       # (blocks, 64, K, 4)
    nb, _, K, _ = b.shape
    b = np.moveaxis(b, 2, 1) if view_major else b            # (blocks, K, 64, 4) | (blocks, 64, K, 4)
    b = b.reshape(nb, 64 * K // 8, 8, 4)
    return distinct(np.moveaxis(b, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--chunk-rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    NV, SN, CR = 3, args.samples, args.chunk_rays
    fr = make_frame(512, 640, NV, seed=0)
    n_rays = fr.H * fr.W
    starts = [int(i * (n_rays // CR) / args.chunks) * CR for i in range(args.chunks)]
    poses = fr.batch["source_poses"][0]
    nf = fr.batch["near_fars"][0][0]
    U1, U2 = sampler_uniforms(0, SN, SN, n_rays)
    acc = {}
    for s in starts:
        idx = torch.arange(s, s + CR)
        ray_d = fr.batch["ray_d"][0][:, idx].t().contiguous()
        ray_o = fr.batch["ray_o"][0][None].expand(CR, 3).contiguous()
        cz = fr.batch["cam_ray_d"][0][2, idx]
        near, far = nf[0] / cz, nf[1] / cz
        _, z = O.fixed_sample(ray_o, ray_d, near, far, U1[:, idx])
        mid = (0.5 * (near + far))[:, None]
        sigma = 2.0 * ((far - near) / (SN - 1))[:, None]
        passes = {"coarse": z,
                  "fine, surface": O.importance_sample(ray_o, ray_d, torch.exp(-0.5 * ((z - mid) / sigma) ** 2), z, U2[:, idx])[1],
                  "fine, flat": O.importance_sample(ray_o, ray_d, torch.ones_like(z), z, U2[:, idx])[1]}
        for pname, zz in passes.items():
            pts = ray_o[:, None, :] + zz[:, :, None] * ray_d[:, None, :]
            xy, xyz, _ = O.project(poses, pts, (nf[0], nf[1]))
            xy, zn = xy.double().numpy(), xyz[..., 2].double().numpy()
            fams = phase_a(fr, xy, zn)
            feat, sim_a, sim_b = coop(fr, xy, NV)
            for R, S in SHAPES:
                key = f"{R}x{S}"
                for fname, a in fams.items():                # lanes of a wave: the 64 local points of ONE view
                    acc.setdefault((pname, fname), {}).setdefault(key, []).append(distinct(np.moveaxis(waves(a, R, S), 1, -1)))
                for order, vm in (("point-major", False), ("view-major", True)):
                    acc.setdefault((pname, f"image features, {order} items"), {}).setdefault(key, []).append(coop_lines(feat, R, S, vm))
                    acc.setdefault((pname, f"pair similarities, {order} items"), {}).setdefault(key, []).append(
                        0.5 * (coop_lines(sim_a, R, S, vm) + coop_lines(sim_b, R, S, vm)))
    keys = [f"{R}x{S}" for R, S in SHAPES]
    mean = {k: {c: float(np.mean(v)) for c, v in d.items()} for k, d in acc.items()}
    sep = " | " if args.markdown else "  "
    head = sep.join([f"{'pass':14s}", f"{'load instruction':38s}"] + [f"{k:>6s}" for k in keys])
    print(("| " + head + " |") if args.markdown else head)
    if args.markdown:
        print("|" + "---|" * (2 + len(keys)))
    for (pname, fname), d in mean.items():
        row = sep.join([f"{pname:14s}", f"{fname:38s}"] + [f"{d[k]:6.1f}" for k in keys])
        print(("| " + row + " |") if args.markdown else row)
    # Line accesses per point, all views.  Phase A: NV waves x n instructions x lines / 64 points (n = 4 colour, 4 depth, 24 per
    # frustum).  Cooperative: 64 K / 8 instructions x 4 corners per block, i.e. K / 2 x lines per point, K = NV items (features)
    # or 2 npair sides (similarities).
    npair = NV * (NV - 1) // 2
    print()
    for pname in passes:
        for order in ("point-major", "view-major"):
            tot = {}
            for k in keys:
                t = 0.0
                for (pn, fname), d in mean.items():
                    if pn != pname:
                        continue
                    if "items" in fname:
                        if order in fname:
                            t += (NV if "features" in fname else 2 * npair) / 2 * d[k]
                    else:
                        t += NV * (24 if "frustum" in fname else 4) * d[k] / 64.0
                tot[k] = t
            print(f"{pname:14s} line accesses per point, {order:11s} items: " + "  ".join(f"{k} {tot[k]:6.1f}" for k in keys))


if __name__ == "__main__":
    main()
