"""A custom scene (BlendedMVS, MVImgNet, the output of `python -m uforecon_amd.colmap2mvsnet`) as the batches the model reads: the
reference's `GeneralFit` (code1/dataset/general_fit.py), without OpenCV, einops or a `DataLoader`.

    scan = GeneralScan(test_dir, "scene0", n_views=3, test_ref_view=[0, 1, 2], dataset="mvimage", use_mask=True, device="cuda:0")
    for batch in scan:                      # one batch per kept entry of <test_dir>/scene0/cams/pair.txt, collated batch of one
        net.extract_geometry(batch, out_dir=...)

`GeneralScan` holds the directory layout, the list of entries and the argument checks; what the reference does once an entry's
files are read is `dtu_scan.ViewGroup`, which `DtuScan` shares (general_fit.py repeats dtu_test_sparse.py).  Who computes what
 is that class's split: every 4x4 on the host in the reference's numpy / CPU-torch calls, order and dtypes
(`cameras`); per pixel on the device: the images through `ops.image_resize_u8`, or `ops.image_resize_mask_u8` when a foreground
mask applies, the two ray tables through `ops.pixel_rays`.  With ``device="cpu"`` the host forms of `host_forms` stand in.

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

Restated, not compared: `cameras.decompose_projection_matrix`, `host_forms.resize_u8` and the mask's grey level
(`host_forms.imread_gray`): see there.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import cameras
from .clean_mesh import projection
from .dtu_scan import ViewGroup
from .host_forms import imread_gray, imread_rgb

OFFSET_DIST = 0.0     # general_fit.py:43
DATASET_WH = {"blendedmvs": (768, 576), "mvimage": (960, 544)}      # general_fit.py:59-62


def read_cam_file(filename):
    """general_fit.py:112-134: (P = K_4x4 @ E float32, near, far, depth_min, depth_interval * 1.06) of a `%08d_cam.txt`; near
    and far are the first and the last token of the depth line."""
    K, E, depth = cameras.read_cam_file(filename)
    return projection(K, E), depth[0], depth[-1], depth[0], depth[1] * 1.06


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
        self.homo_pixel = cameras.homo_pixels(self.img_wh[1], self.img_wh[0])

    # ---- general_fit.py:88-109
    def build_list(self):
        metas = []
        for ref_view, src_views in cameras.read_pair_file(os.path.join(self.data_dir, "cams", "pair.txt")):
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
        sample = self.group(idx).batch(0)
        sample["meta"] = ["%s-%s-refview%d" % (self.root_dir.split("/")[-1], self.scan_id, self.metas[idx][0])]
        return sample

    # ---- general_fit.py:299-347, :159-213
    def group(self, idx):
        """`metas[idx]` as the `ViewGroup` of its views, read from the scene's files; the render view is the first."""
        view_ids = self.view_ids(idx)
        masked = self.use_mask and self.dataset != "blendedmvs"
        world_mats, raw_near_fars = [], []
        for vid in view_ids:           # depth_min / depth_interval: the last file's
            P, near, far, depth_min, depth_interval = read_cam_file(os.path.join(self.data_dir, "cams/{:0>8}_cam.txt".format(vid)))
            raw_near_fars.append(np.array([near, far]))
            world_mats.append(P)
        image = "blended_images/{:0>8}_masked.jpg" if self.dataset == "blendedmvs" else "images/{:0>8}.jpg"
        raw = [imread_rgb(os.path.join(self.data_dir, image.format(vid))) for vid in view_ids]
        masks = [imread_gray(os.path.join(self.data_dir, "masks", "{:0>8}_mask.jpg".format(vid))) for vid in view_ids] if masked else None
        if masked and any(m.shape != r.shape[:2] for m, r in zip(masks, raw)):
            raise ValueError(f"GeneralScan: a mask of {self.data_dir} differs in size from its image")
        return ViewGroup(world_mats, raw, masks, [(r.shape[1], r.shape[0]) for r in raw], self.img_wh, [0, 0, 0, 0],
                         np.stack(raw_near_fars), OFFSET_DIST, depth_min, depth_interval, self.ndepths, self.device, self.homo_pixel)
