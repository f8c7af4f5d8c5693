"""The DTU training layout as the batches the model trains and validates on: the reference's `MVSDataset`
(code1/dataset/dtu_train.py:80-498) without OpenCV, torchvision or a `DataLoader`.

    ds = DtuTrain(root, "test", n_views=3, split_filepath="lists/test.txt", test_ref_views=[23, 24, 33], device="cuda:0")
    for batch in ds:                         # the collated batch-of-one form: every tensor with a leading 1, meta a list
        parts.append(net.validation_step(batch))

The tree: `Cameras/train/%08d_cam.txt` (all 49 are read), `Cameras/pair.txt`, `Rectified/<scan>_train/rect_%03d_<light>_r5000.png`
(640x512, used as they are) and `Depths_raw/<scan>/depth_map_%04d.pfm` (1600x1200).

Who computes what, as in `dtu_scan`: every 4x4 on the host, in the reference's calls, order and dtypes (`cameras`);
everything per pixel on the device, through `host_forms.image_planes` / `pixel_rays` and `depth_gt` below -- the pictures
(`ops.image_resize_u8` at equal sizes: the identity on the bytes, then / 255), the ray table `ray_d` (`ops.pixel_rays`) and
the ground-truth depths (`ops.depth_gt_prepare`).  With ``device="cpu"`` their host forms stand in (`depth_gt_host` here).  `cam_ray_d` is always the host's float64 table
(`host_forms.pixel_rays64`): the depths divide by its z row.

Kept quirks of the reference (tests/golden/dtu_train_small.npz went through its own code): `depth_min` / `depth_interval`
(x 1.06) are those of the LAST camera file read (view 48); with `test_ref_views` the source list of a 'val' / 'test' item is that
list itself, the reference view included; `proj_matrices` holds the unscaled world-to-camera matrices of the sources and leaves
[1, 3, 3] zero; near / far are recomputed from the scaled cameras; the header scale of a PFM file is ignored.

One deliberate difference: the reference leaves `ray_d`, `cam_ray_d` and `depths_h` in float64 (its ray tables are products
with a float64 pixel table and nothing casts them); every consumer here reads float32, so the loader returns the float32
rounding of those values -- `depths_h` is the reference's float64 quotient `depth * scale_factor / cam_ray_d.z` rounded once.
`view_selection_type="random"` draws from `random.Random(seed)` instead of the process-wide generator: reproducible.
"""
from __future__ import annotations

import os
import random
import re

import numpy as np
import torch

from . import cameras
from ._lib import MAX_VIEWS, UfrError
from .host_forms import image_planes, imread_rgb, pixel_rays, pixel_rays64

NUM_ALL_IMGS = 49                       # dtu_train.py:96
PFM_CROP = (44, 80)                     # dtu_train.py:253: rows 44..556, columns 80..720 of the half-size depth map


def read_pfm_rows(filename):
    """A grey PFM file as (rows (Hs,Ws) float32 in FILE order, bottom_up): read_pfm (dtu_train.py:18-53) without its flip --
    the file stores the bottom row first, which `ufr_depth_gt_prepare` / `depth_gt_host` undo."""
    with open(filename, "rb") as f:
        header = f.readline().decode("utf-8").rstrip()
        if header != "Pf":
            raise ValueError(f"{filename}: not a grey PFM file (header {header!r})")
        dims = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if not dims:
            raise ValueError(f"{filename}: malformed PFM header")
        width, height = map(int, dims.groups())
        endian = "<" if float(f.readline().rstrip()) < 0 else ">"
        data = np.fromfile(f, endian + "f")
    return np.ascontiguousarray(data.reshape(height, width).astype(np.float32)), True


def depth_gt_host(pfm_rows, bottom_up, y0, x0, H, W, scale_factor, cam_ray_z):
    """ufr_depth_gt_prepare on the host, in the reference's calls: flip, nearest half-size picture (source pixel (2y, 2x)), crop,
    x scale_factor in float32, / cam_ray_d.z in float64, rounded to float32.  -> (H,W) float32 array."""
    data = np.asarray(pfm_rows, np.float32)
    if bottom_up:
        data = np.flipud(data)
    Hh, Wh = int(np.rint(data.shape[0] * 0.5)), int(np.rint(data.shape[1] * 0.5))
    if y0 < 0 or x0 < 0 or H < 1 or W < 1 or y0 + H > Hh or x0 + W > Wh:
        raise ValueError(f"depth_gt_host: the crop {H}x{W} at ({y0}, {x0}) leaves the half-size picture {Hh}x{Wh}")
    crop = data[0::2, 0::2][y0:y0 + H, x0:x0 + W]
    scaled = crop * np.float32(scale_factor)                                                    # dtu_train.py:429
    return (scaled.astype(np.float64).reshape(-1) / np.asarray(cam_ray_z, np.float64).reshape(-1)).astype(np.float32).reshape(H, W)


def depth_gt(device, pfm_rows, bottom_up, y0, x0, H, W, scale_factor, cam_ray_z):
    """The (H,W) float32 ground-truth ray depth on ``device`` from a PFM file's rows (a host array); ``cam_ray_z`` (H*W float64)
    is a tensor on ``device``."""
    device = torch.device(device)
    if device.type == "cuda":
        from . import ops

        with torch.cuda.device(device):
            return ops.depth_gt_prepare(torch.from_numpy(pfm_rows).to(device), bottom_up, y0, x0, H, W, scale_factor, cam_ray_z)
    return torch.from_numpy(depth_gt_host(pfm_rows, bottom_up, y0, x0, H, W, scale_factor, cam_ray_z.numpy())).to(device)


def read_cam_file(filename):
    """dtu_train.py:211-233: (intrinsics 4x4 float32, extrinsics 4x4 float32, [depth_min, depth_max], depth_min, interval * 1.06)."""
    K, E, depth = cameras.read_cam_file(filename)
    intrinsics = np.float32(np.diag([1, 1, 1, 1]))
    intrinsics[:3, :3] = K
    return intrinsics, E, [depth[0], depth[0] + depth[1] * 192], depth[0], depth[1] * 1.06


class DtuTrain:
    """See the module text.  ``len()`` = the number of (light, scan, reference view) items; ``ds[i]`` is item ``i``'s batch."""

    def __init__(self, root_dir, split, n_views=3, img_wh=(640, 512), split_filepath=None, scans=None, pair_filepath=None,
                 test_ref_views=(), view_selection_type="best", ndepths=192, device="cuda", seed=0):
        self.root_dir, self.split, self.n_views, self.ndepths = str(root_dir), split, int(n_views), ndepths
        self.device = torch.device(device)
        self.img_W, self.img_H = int(img_wh[0]), int(img_wh[1])
        if self.img_W % 32 or self.img_H % 32:
            raise ValueError("img_wh must both be multiples of 32!")
        if split not in ("train", "val", "test"):
            raise ValueError(f"DtuTrain: split {split!r} (train, val or test)")
        if view_selection_type not in ("best", "random"):
            raise NotImplementedError(view_selection_type)
        self.test_ref_views = list(test_ref_views)
        self.view_selection_type, self._rng = view_selection_type, random.Random(seed)
        if scans is None:
            if split_filepath is None:
                raise ValueError("DtuTrain: split_filepath or scans is required")
            with open(split_filepath) as f:
                scans = [line.rstrip() for line in f.readlines()]
        self.scans = list(scans)
        self.pair_filepath = pair_filepath if pair_filepath is not None else os.path.join(self.root_dir, "Cameras", "pair.txt")
        self.metas, self.ref_src_pairs = self.build_metas()
        most = max((len(self._view_ids(m)) - 1 for m in self.metas), default=0)
        if most > MAX_VIEWS:
            raise UfrError(f"DtuTrain: {most} source views per item, the ray path takes at most {MAX_VIEWS} (UFR_MAX_VIEWS)")
        self.all_intrinsics, self.all_extrinsics, self.all_near_fars = [], [], []
        for vid in range(NUM_ALL_IMGS):           # dtu_train.py:235-243; depth_min / depth_interval: the last file's
            K, E, near_far, self.depth_min, self.depth_interval = read_cam_file(
                os.path.join(self.root_dir, f"Cameras/train/{vid:08d}_cam.txt"))
            K[:2] *= 4
            self.all_intrinsics.append(K)
            self.all_extrinsics.append(E)
            self.all_near_fars.append(near_far)
        self.homo_pixel = cameras.homo_pixels(self.img_H, self.img_W)
        self._cam_rays = {}                       # bytes of the normalised intrinsics' inverse -> (cam_ray_d float32, z float64)

    # ---- dtu_train.py:160-208
    def build_metas(self):
        metas = []
        light_idxs = [3] if "train" not in self.split else range(7)
        pairs = cameras.read_pair_file(self.pair_filepath)
        for light_idx in light_idxs:
            for scan in self.scans:
                for ref_view, src_views in pairs:
                    if self.view_selection_type == "random":
                        src_views = self._rng.sample([i for i in range(49) if i != ref_view], self.n_views - 1)
                    if self.split != "train" and len(self.test_ref_views) > 0:
                        if ref_view not in self.test_ref_views:
                            continue
                        src_views = self.test_ref_views
                    metas.append((scan, light_idx, ref_view, list(src_views)))
        return metas, dict(pairs)

    def _view_ids(self, meta):
        _, _, ref_view, src_views = meta
        return [ref_view] + (src_views[:self.n_views - 1] if self.split == "train" else src_views)     # dtu_train.py:322-325

    def __len__(self):
        return len(self.metas)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def _cam_ray_d(self, m_inv):
        key = m_inv.numpy().tobytes()
        if key not in self._cam_rays:
            if len(self._cam_rays) >= 4:
                self._cam_rays.clear()
            d64 = pixel_rays64(m_inv, self.homo_pixel)
            self._cam_rays[key] = (d64.float().to(self.device), d64[2].contiguous().to(self.device))
        return self._cam_rays[key]

    # ---- dtu_train.py:318-498
    def __getitem__(self, idx):
        return self.finish(idx, self.load(idx))

    def load(self, idx):
        """The files of item ``idx``, decoded: (its pictures (uint8 arrays), its depth maps' (rows, bottom_up)).  Host work on
        host memory that touches no state of the loader, so a worker thread may run it ahead of `finish` (train.Prefetch)."""
        meta = self.metas[idx % len(self.metas)]
        scan, light_idx, _, _ = meta
        raw, depths = [], []
        for vid in self._view_ids(meta):
            img = imread_rgb(os.path.join(self.root_dir, f"Rectified/{scan}_train/rect_{vid + 1:03d}_{light_idx}_r5000.png"))
            if img.shape != (self.img_H, self.img_W, 3):
                raise ValueError(f"DtuTrain: {scan} view {vid} is {img.shape[1]}x{img.shape[0]}, expected {self.img_W}x{self.img_H}")
            raw.append(img)
            depth_filename = os.path.join(self.root_dir, f"Depths_raw/{scan}/depth_map_{vid:04d}.pfm")
            if os.path.exists(depth_filename):
                depths.append(read_pfm_rows(depth_filename))
        return raw, depths

    def finish(self, idx, loaded):
        """Item ``idx``'s batch from its decoded files: ``ds[idx]`` is ``ds.finish(idx, ds.load(idx))``."""
        meta = self.metas[idx % len(self.metas)]
        scan, light_idx, ref_view, _ = meta
        view_ids = self._view_ids(meta)
        raw, depth_rows = loaded
        w2c_ref_inv = np.linalg.inv(self.all_extrinsics[ref_view])
        intrinsics = [self.all_intrinsics[vid] for vid in view_ids]
        w2cs = [self.all_extrinsics[vid] @ w2c_ref_inv for vid in view_ids]
        near_fars = [self.all_near_fars[vid] for vid in view_ids]
        depth_max = self.depth_interval * self.ndepths + self.depth_min
        depth_values_org_scale = np.arange(self.depth_min, depth_max, self.depth_interval, dtype=np.float32)
        proj_matrices = cameras.proj_matrices_ms(np.stack([self.all_extrinsics[vid] for vid in view_ids[1:]]), np.stack(intrinsics[1:]))

        # cal_scale_mat (dtu_train.py:299-307)
        center, radius, _ = cameras.get_boundingbox([self.img_H, self.img_W], torch.from_numpy(np.stack(intrinsics)),
                                                    torch.from_numpy(np.stack(w2cs)), near_fars)
        scale_mat, scale_factor = cameras.scale_matrix(center, radius)
        scaled = [cameras.scaled_camera((intrinsic @ extrinsic @ scale_mat)[:3, :4]) for intrinsic, extrinsic in zip(intrinsics, w2cs)]
        intrinsics = np.stack(intrinsics)
        w2cs, c2ws, near_fars = (np.stack(x) for x in zip(*scaled))

        s = {}
        s["w2cs"] = torch.from_numpy(w2cs.astype(np.float32))
        s["c2ws"] = torch.from_numpy(c2ws.astype(np.float32))
        s["near_fars"] = torch.from_numpy(near_fars.astype(np.float32))
        s["intrinsics"] = torch.from_numpy(intrinsics.astype(np.float32))[:, :3, :3]
        s["scale_mat"] = torch.from_numpy(scale_mat)
        s["trans_mat"] = torch.from_numpy(w2c_ref_inv)
        intrinsics_pad = cameras.pad_intrinsics(s["intrinsics"])
        normalize_matrix = cameras.normalize_matrix(self.img_H, self.img_W)
        s["ref_pose"] = normalize_matrix @ (intrinsics_pad @ s["w2cs"])[0]
        s["source_poses"] = normalize_matrix @ (intrinsics_pad @ s["w2cs"])[1:]
        s["ref_pose_inv"] = torch.inverse(s["ref_pose"])
        s["source_poses_inv"] = torch.inverse(s["source_poses"])
        s["ray_o"] = s["ref_pose_inv"][:3, -1]
        s["depth_values_org_scale"] = torch.from_numpy(depth_values_org_scale)
        s["scale_factor"] = torch.as_tensor(scale_factor)
        batch = {k: v.contiguous()[None].to(self.device) for k, v in s.items()}

        cam_ray_d, cam_ray_z = self._cam_ray_d(torch.inverse(normalize_matrix @ intrinsics_pad[0]))
        ray_d = pixel_rays(self.device, s["ref_pose_inv"], self.img_H, self.img_W, s["ray_o"], self.homo_pixel)
        images = image_planes(self.device, np.stack(raw), self.img_H, self.img_W)
        batch["images"] = images[None]
        batch["ref_img"], batch["source_imgs"] = images[0][None], images[1:][None]
        batch["ray_d"], batch["cam_ray_d"] = ray_d[None], cam_ray_d[None]
        y0, x0 = PFM_CROP
        batch["depths_h"] = torch.stack([depth_gt(self.device, rows, bottom_up, y0, x0, self.img_H, self.img_W,
                                                  float(np.float32(scale_factor)), cam_ray_z) for rows, bottom_up in depth_rows])[None]
        batch["proj_matrices"] = {k: torch.from_numpy(v)[None].to(self.device) for k, v in proj_matrices.items()}
        batch["meta"] = [str(scan) + "_light" + str(light_idx) + "_refview" + str(ref_view)]
        return batch
