"""A custom scene (BlendedMVS, MVImgNet, the output of `python -m uforecon_amd.colmap2mvsnet`) as the batches the model reads: the
reference's `GeneralFit` (code1/dataset/general_fit.py), without OpenCV, einops or a `DataLoader`.

    scan = GeneralScan(test_dir, "scene0", n_views=3, test_ref_view=[0, 1, 2], dataset="mvimage", use_mask=True, device="cuda:0")
    for batch in scan:                      # one batch per kept entry of <test_dir>/scene0/cams/pair.txt, collated batch of one
        net.extract_geometry(batch, out_dir=...)

Who computes what is `dtu_scan.DtuScan`'s split: every 4x4 on the host in the reference's numpy / CPU-torch
calls, order and dtypes (`load_K_Rt_from_P`, `get_boundingbox`, the scaled cameras, the poses -- the functions of dtu_scan.py,
which general_fit.py repeats); per pixel on the device: the images through `ops.image_resize_u8`, or `ops.image_resize_mask_u8`
when a foreground mask applies, the two ray tables through `ops.pixel_rays`.  With ``device="cpu"`` the host forms of
dtu_scan.py stand in (`image_planes_host`, `image_mask_planes_host`, `pixel_rays_host`).

Quirks of the reference that are kept (tests/golden/general_scan_small.npz has them):

  * `metas` keeps the entries of ``cams/pair.txt`` whose reference view is in ``test_ref_view``, and REPLACES their sources by
    the whole ``test_ref_view`` list: ``view_ids = [ref] + test_ref_view[:n_views - 1]`` may hold the reference view twice.  With
    an empty ``test_ref_view`` every entry is kept with its own sources;
  * `depth_min` and `depth_interval` (x 1.06) are those of the LAST camera file read; the raw near / far of a view are the
    first and the last token of its file's depth line, and drive the bounding box (factor 1.1);
  * the render camera is the source camera (`offset_dist` 0), and the render view is always the first of `view_ids`;
  * the image size follows the dataset: ``blendedmvs`` 768x576 from ``blended_images/%08d_masked.jpg``, ``mvimage`` 960x544 from
    ``images/%08d.jpg`` with ``masks/%08d_mask.jpg``; the mask is applied only with ``use_mask`` and ``mvimage``, as
    image / 255 x mask / 254;
  * `meta` is ``"%s-%s-refview%d"``; `proj_matrices` holds the unscaled `all_w2cs`; `start_idx` is 0.

Ours: ``img_wh`` overrides the dataset's size (tests need small pictures); a scan whose entries cannot fill ``n_views`` is
refused when it is opened (the reference fails with an IndexError in its first batch).

Restated, not compared: `dtu_scan.decompose_projection_matrix` and `dtu_scan.resize_u8` (see there), and the mask's grey
level -- a mask file with one channel (PIL mode "L") is read as it is; any other file is reduced with PIL's ``convert("L")``,
the ITU-R 601-2 luma L = (299 R + 587 G + 114 B) / 1000 of its RGB form in PIL's integer arithmetic.  cv2.imread(path, 0)
decodes a colour JPEG straight to its luma plane and weighs a colour PNG with its own fixed-point constants, so a colour
mask may differ from the reference's by a grey level; a single-channel mask does not.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .dtu_scan import (DtuScan, get_boundingbox, homo_pixels, image_mask_planes_host, image_planes_host, imread_rgb,
                       load_K_Rt_from_P)

OFFSET_DIST = 0.0     # general_fit.py:43
DATASET_WH = {"blendedmvs": (768, 576), "mvimage": (960, 544)}      # general_fit.py:59-62


def imread_gray(path):
    """A mask file as (H, W) uint8: see the module text."""
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im if im.mode == "L" else im.convert("L"), dtype=np.uint8)


def read_pair_file(path):
    """[(ref view, [source views])] of an MVSNet pair file (general_fit.py:88-105 without the filter)."""
    entries = []
    with open(path) as f:
        for _ in range(int(f.readline())):
            ref_view = int(f.readline().rstrip())
            entries.append((ref_view, [int(x) for x in f.readline().rstrip().split()[1::2]]))
    return entries


def read_cam_file(filename):
    """general_fit.py:112-134: (P = K_4x4 @ E float32, near, far, depth_min, depth_interval * 1.06) of a `%08d_cam.txt`; near
    and far are the first and the last token of the depth line."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.fromstring(" ".join(lines[1:5]), dtype=np.float32, sep=" ").reshape((4, 4))
    intrinsics = np.fromstring(" ".join(lines[7:10]), dtype=np.float32, sep=" ").reshape((3, 3))
    intrinsics_ = np.float32(np.diag([1, 1, 1, 1]))
    intrinsics_[:3, :3] = intrinsics
    tokens = lines[11].split()
    near, far = float(tokens[0]), float(tokens[-1])
    return intrinsics_ @ extrinsics, near, far, near, float(tokens[1]) * 1.06


class _ViewGroup(DtuScan):
    """One entry of `metas` as a `DtuScan` of its views: the constructor and the scene loading are general_fit.py's
    (:299-347, :159-213), everything after them is shared."""

    def __init__(self, scan, view_ids):  # noqa: D107 -- DtuScan.__init__ reads DTU's directory layout and is not called
        self.root_dir, self.scan_id, self.n_views, self.ndepths = scan.root_dir, scan.scan_id, scan.n_views, scan.ndepths
        self.device, self.data_dir = scan.device, scan.data_dir
        self.idx = list(view_ids)
        self.clip_wh = [0, 0, 0, 0]
        self.world_mats_np, self.images_list, self.masks_list, raw_near_fars = [], [], [], []
        for vid in self.idx:           # depth_min / depth_interval: the last file's
            if scan.dataset == "blendedmvs":
                self.images_list.append(os.path.join(self.data_dir, "blended_images/{:0>8}_masked.jpg".format(vid)))
            else:
                self.images_list.append(os.path.join(self.data_dir, "images/{:0>8}.jpg".format(vid)))
                self.masks_list.append(os.path.join(self.data_dir, "masks", "{:0>8}_mask.jpg".format(vid)))
            P, near, far, self.depth_min, self.depth_interval = read_cam_file(os.path.join(self.data_dir, "cams/{:0>8}_cam.txt".format(vid)))
            raw_near_fars.append(np.array([near, far]))
            self.world_mats_np.append(P)
        self.raw_near_fars = np.stack(raw_near_fars)
        self.ref_w2c = np.linalg.inv(load_K_Rt_from_P(self.world_mats_np[0][:3, :4])[1])
        self._load_scene(list(scan.img_wh), scan.use_mask and len(self.masks_list) > 0)
        self.img_W, self.img_H = self.img_wh
        # general_fit.py:340-347, :216-223
        center, radius, _ = get_boundingbox([self.img_H, self.img_W], self.all_intrinsics, self.all_w2cs, self.raw_near_fars)
        radius = radius * 1.1
        scale_mat = np.diag([radius, radius, radius, 1.0])
        scale_mat[:3, 3] = center.cpu().numpy()
        self.scale_mat = scale_mat.astype(np.float32)
        self.scale_factor = 1. / radius.cpu().numpy()
        self._scale_cam_info()
        self.homo_pixel = scan.homo_pixel
        self._shared = None

    def _planes(self, raw, masks, img_wh):
        H, W = img_wh[1], img_wh[0]
        if self.device.type == "cuda":
            from . import ops

            with torch.cuda.device(self.device):
                dev = lambda a: torch.from_numpy(a).to(self.device)  # noqa: E731
                return ops.image_resize_u8(dev(raw), H, W) if masks is None else ops.image_resize_mask_u8(dev(raw), dev(masks), H, W)
        planes = image_planes_host(raw, H, W) if masks is None else image_mask_planes_host(raw, masks, H, W)
        return torch.from_numpy(planes).to(self.device)

    # ---- general_fit.py:159-213
    def _load_scene(self, img_wh, masked):
        raw = [imread_rgb(p) for p in self.images_list]
        masks = [imread_gray(p) for p in self.masks_list] if masked else None
        if masked and any(m.shape != r.shape[:2] for m, r in zip(masks, raw)):
            raise ValueError(f"GeneralScan: a mask of {self.data_dir} differs in size from its image")
        if all(r.shape == raw[0].shape for r in raw):      # one launch for the views of one size, else one per view
            self.all_images = self._planes(np.stack(raw), np.stack(masks) if masked else None, img_wh)
        else:
            self.all_images = torch.cat([self._planes(r[None], masks[k][None] if masked else None, img_wh) for k, r in enumerate(raw)])
        intr, w2cs, render_w2cs, w2cs_org, render_w2cs_org = [], [], [], [], []
        for P, image in zip(self.world_mats_np, raw):
            original_h, original_w, _ = image.shape
            scale_x = img_wh[0] / original_w
            scale_y = img_wh[1] / original_h
            intrinsics, c2w = load_K_Rt_from_P(P[:3, :4])
            w2c = np.linalg.inv(c2w)
            render_c2w = c2w.copy()
            render_c2w[:3, 3] += render_c2w[:3, 0] * OFFSET_DIST
            render_w2c = np.linalg.inv(render_c2w)
            intrinsics[:1] *= scale_x
            intrinsics[1:2] *= scale_y
            intrinsics[0, 2] -= self.clip_wh[0]
            intrinsics[1, 2] -= self.clip_wh[1]
            intr.append(intrinsics)
            w2cs.append(w2c @ np.linalg.inv(self.ref_w2c))        # world -> the first camera's system
            render_w2cs.append(render_w2c @ np.linalg.inv(self.ref_w2c))
            w2cs_org.append(w2c)
            render_w2cs_org.append(render_w2c)
        f32 = lambda xs: torch.from_numpy(np.stack(xs)).to(torch.float32)  # noqa: E731
        self.all_intrinsics, self.all_w2cs, self.all_render_w2cs = f32(intr), f32(w2cs), f32(render_w2cs)
        self.all_w2cs_original, self.all_render_w2cs_original = f32(w2cs_org), f32(render_w2cs_org)
        self.img_wh = [img_wh[0], img_wh[1]]


class GeneralScan:
    """See the module text.  ``len()`` = ``len(metas)``; ``scan[i]`` is the batch of ``metas[i]`` (tensors on ``device``)."""

    def __init__(self, root_dir, scan_id, n_views=3, test_ref_view=None, dataset="blendedmvs", use_mask=False, img_wh=None,
                 ndepths=192, device="cuda"):
        self.root_dir, self.scan_id, self.n_views, self.ndepths = str(root_dir), str(scan_id), int(n_views), ndepths
        self.device = torch.device(device)
        self.dataset, self.use_mask = dataset, bool(use_mask)
        self.test_ref_view = list(test_ref_view) if test_ref_view is not None else []
        if dataset not in DATASET_WH:
            raise ValueError(f"GeneralScan: dataset {dataset!r} (one of {sorted(DATASET_WH)})")
        self.img_wh = [int(v) for v in (img_wh if img_wh is not None else DATASET_WH[dataset])]
        if self.img_wh[0] < 2 or self.img_wh[1] < 2 or self.n_views < 1:
            raise ValueError(f"GeneralScan: {self.n_views} views of {self.img_wh[1]}x{self.img_wh[0]} pixels")
        self.data_dir = os.path.join(self.root_dir, self.scan_id)
        self.metas = self.build_list()
        for ref_view, src_views in self.metas:
            if 1 + len(src_views) < self.n_views:
                raise ValueError(f"GeneralScan: {self.n_views} views asked, reference view {ref_view} of {self.data_dir} has "
                                 f"{len(src_views)} source views ({'--test_ref_view' if self.test_ref_view else 'cams/pair.txt'})")
        self.homo_pixel = homo_pixels(self.img_wh[1], self.img_wh[0])

    # ---- general_fit.py:88-109
    def build_list(self):
        metas = []
        for ref_view, src_views in read_pair_file(os.path.join(self.data_dir, "cams", "pair.txt")):
            if len(self.test_ref_view) > 0:
                if ref_view not in self.test_ref_view:
                    continue
                src_views = self.test_ref_view
            metas.append((ref_view, src_views))
        return metas

    def __len__(self):
        return len(self.metas)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def view_ids(self, idx):
        ref_view, src_views = self.metas[idx]
        return [ref_view] + list(src_views[:self.n_views - 1])

    def __getitem__(self, idx):
        if not -len(self.metas) <= idx < len(self.metas):
            raise IndexError(idx)
        group = _ViewGroup(self, self.view_ids(idx))
        sample = DtuScan.__getitem__(group, 0)
        sample["meta"] = ["%s-%s-refview%d" % (self.root_dir.split("/")[-1], self.scan_id, self.metas[idx][0])]
        return sample
