"""A DTU test scan as the batches the model reads: the reference's `DtuFitSparse` (code1/dataset/dtu_test_sparse.py:75-436),
without OpenCV, torchvision or a `DataLoader`.

    scan = DtuScan(test_dir, "scan24", n_views=3, test_view_pair=[23, 24, 33], device="cuda:0")
    for batch in scan:                      # one batch per render view, in the collated batch-of-one form
        net.extract_geometry(batch, out_dir=...)

`DtuScan` holds the directory layout, the view list and the argument checks, and hands what it read to `ViewGroup`: everything
the reference does once its files are read, which `general_scan.GeneralScan` shares (general_fit.py repeats it).

Who computes what:

  host    every 4x4: the camera files, the decomposition, inverses, the bounding box, the scaled cameras, the poses -- the
          numpy / CPU-torch calls of `cameras` in the reference's order and dtypes (the reference runs them on the CPU as well),
          so these entries equal the reference's bit for bit (tests/golden/dtu_scan_small.npz went through its own code);
  device  everything per pixel: the images and the two ray tables, through `host_forms.image_planes` / `pixel_rays` (the
          kernels `ops.image_resize_u8` and `ops.pixel_rays`; with ``device="cpu"`` their host forms).

Quirks of the reference that are kept (the goldens have them): `depth_min` and `depth_interval` (x 1.06) are those of the LAST
camera file read; `depth_values_org_scale` is `np.arange(min, max, interval, float32)` whatever its length; the render camera
is the source camera moved 25 mm along its own x axis; `proj_matrices` holds the UNSCALED `all_w2cs` and leaves [1, 3, 3] zero;
the ray tables are computed in float64 and cast at the end; scan-level tensors are shared between the batches of one scan.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import cameras
from .clean_mesh import SET1_VIEWS, projection
from .host_forms import image_planes, imread_rgb, pixel_rays

OFFSET_DIST = 25      # mm, dtu_test_sparse.py:88


def read_cam_file(filename):
    """dtu_test_sparse.py:185-206: (P = K_4x4 @ E float32, depth_min, depth_interval * 1.06) of a `%08d_cam.txt`."""
    K, E, depth = cameras.read_cam_file(filename)
    return projection(K, E), depth[0], depth[1] * 1.06


class ViewGroup:
    """The views one batch is made of, from what a loader read: dtu_test_sparse.py:247-436 (general_fit.py:159-347).

    ``world_mats``: one P = K_4x4 @ E per view, the first view's camera is the group's frame; ``images`` (and ``masks``): the
    decoded pictures, (Hs,Ws,3) (and (Hs,Ws)) uint8, which may differ in size; ``original_whs``: per view, the size its
    intrinsics refer to; ``img_wh``: the size every picture is resized to, ``clip`` (left, top, right, bottom) cut off after;
    ``raw_near_fars``: per view, the depth range that bounds the scene, in the caller's own dtype; ``offset_dist``: how far the
    render camera stands from the source camera along its x axis; ``homo_pixel``: `cameras.homo_pixels` of the clipped size.
    ``batch(i)`` is the batch that renders view ``i`` (tensors on ``device``, no `meta`)."""

    def __init__(self, world_mats, images, masks, original_whs, img_wh, clip, raw_near_fars, offset_dist, depth_min, depth_interval,
                 ndepths, device, homo_pixel):
        self.n_views, self.device, self.homo_pixel = len(world_mats), torch.device(device), homo_pixel
        self.depth_min, self.depth_interval, self.ndepths = depth_min, depth_interval, ndepths
        self.img_wh = [img_wh[0] - clip[0] - clip[2], img_wh[1] - clip[1] - clip[3]]
        self.img_W, self.img_H = self.img_wh
        H, W = img_wh[1], img_wh[0]
        if all(r.shape == images[0].shape for r in images):      # one launch for the views of one size, else one per view
            self.all_images = image_planes(self.device, np.stack(images), H, W, clip, None if masks is None else np.stack(masks))
        else:
            self.all_images = torch.cat([image_planes(self.device, r[None], H, W, clip, None if masks is None else masks[k][None])
                                         for k, r in enumerate(images)])
        # ---- dtu_test_sparse.py:247-298
        self.ref_w2c = np.linalg.inv(cameras.load_K_Rt_from_P(world_mats[0][:3, :4])[1])
        intr, w2cs, render_w2cs, w2cs_org, render_w2cs_org = [], [], [], [], []
        for P, (original_w, original_h) in zip(world_mats, original_whs):
            intrinsics, c2w = cameras.load_K_Rt_from_P(P[:3, :4])
            w2c = np.linalg.inv(c2w)
            render_c2w = c2w.copy()
            render_c2w[:3, 3] += render_c2w[:3, 0] * offset_dist
            render_w2c = np.linalg.inv(render_c2w)
            intrinsics[:1] *= img_wh[0] / original_w
            intrinsics[1:2] *= img_wh[1] / original_h
            intrinsics[0, 2] -= clip[0]
            intrinsics[1, 2] -= clip[1]
            intr.append(intrinsics)
            w2cs.append(w2c @ np.linalg.inv(self.ref_w2c))        # world -> the first camera's system
            render_w2cs.append(render_w2c @ np.linalg.inv(self.ref_w2c))
            w2cs_org.append(w2c)
            render_w2cs_org.append(render_w2c)
        f32 = lambda xs: torch.from_numpy(np.stack(xs)).to(torch.float32)  # noqa: E731
        self.all_intrinsics, self.all_w2cs, self.all_render_w2cs = f32(intr), f32(w2cs), f32(render_w2cs)
        self.all_w2cs_original, self.all_render_w2cs_original = f32(w2cs_org), f32(render_w2cs_org)
        # ---- dtu_test_sparse.py:301-308
        center, radius, _ = cameras.get_boundingbox([self.img_H, self.img_W], self.all_intrinsics, self.all_w2cs, raw_near_fars)
        self.scale_mat, self.scale_factor = cameras.scale_matrix(center, radius)
        self._scale_cam_info()
        self._shared = None

    # ---- dtu_test_sparse.py:311-376
    def _scaled(self, w2cs):
        """`cameras.scaled_camera` of every view: the stacked float32 (w2cs, c2ws, near_fars)"""
        cams = [cameras.scaled_camera(np.matmul((K @ w2c).numpy(), self.scale_mat)[:3, :4])                   # `tensor @ ndarray`
                for K, w2c in zip(self.all_intrinsics, w2cs)]
        return [torch.from_numpy(np.float32(np.stack(x))) for x in zip(*cams)]

    def _scale_cam_info(self):
        self.scaled_intrinsics = self.all_intrinsics.clone()
        self.scaled_w2cs, self.scaled_c2ws, self.scaled_near_fars = self._scaled(self.all_w2cs)
        self.scaled_render_w2cs, self.scaled_render_c2ws, _ = self._scaled(self.all_render_w2cs)
        self.proj_matrices_ms = cameras.proj_matrices_ms(self.all_w2cs, self.all_intrinsics)

    def _rays(self, m_inv, origin):
        return pixel_rays(self.device, m_inv, self.img_H, self.img_W, origin, self.homo_pixel)

    def _scan_level(self):
        """What every render view of the group shares (dtu_test_sparse.py:387-419 without the view's own entries)."""
        if self._shared is None:
            V = self.n_views
            s = {}
            s["scale_mat"] = torch.from_numpy(self.scale_mat)
            s["trans_mat"] = torch.from_numpy(np.linalg.inv(self.ref_w2c))
            s["w2cs"] = self.scaled_w2cs
            s["intrinsics"] = self.scaled_intrinsics[:, :3, :3]
            depth_max = self.depth_interval * self.ndepths + self.depth_min
            s["depth_values_org_scale"] = torch.from_numpy(np.arange(self.depth_min, depth_max, self.depth_interval, dtype=np.float32))
            s["near_fars"] = self.scaled_near_fars
            s["scale_factor"] = torch.as_tensor(self.scale_factor)
            intrinsics_pad = cameras.pad_intrinsics(s["intrinsics"])
            normalize_matrix = cameras.normalize_matrix(self.img_H, self.img_W)
            s["source_poses"] = normalize_matrix @ (intrinsics_pad @ s["w2cs"])[list(range(V))]
            s["source_poses_inv"] = torch.inverse(s["source_poses"])
            self._ref_poses = intrinsics_pad @ self.scaled_render_w2cs
            self._normalize_matrix = normalize_matrix
            s["cam_ray_d"] = self._rays(torch.inverse(normalize_matrix @ intrinsics_pad[0]), None)
            s = {k: v.contiguous()[None].to(self.device) for k, v in s.items()}
            s["source_imgs"] = self.all_images[None]
            s["proj_matrices"] = {k: torch.from_numpy(v)[None].to(self.device) for k, v in self.proj_matrices_ms.items()}
            s["start_idx"] = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._shared = s
        return self._shared

    def batch(self, render_idx):
        sample = dict(self._scan_level())
        sample["proj_matrices"] = dict(sample["proj_matrices"])
        view = {}
        view["extrinsic_render_view"] = self.all_render_w2cs_original[render_idx]
        view["intrinsic_render_view"] = self.scaled_intrinsics[render_idx, :3, :3]
        view["ref_pose"] = self._normalize_matrix @ self._ref_poses[render_idx]
        view["ref_pose_inv"] = torch.inverse(view["ref_pose"])
        view["ray_o"] = view["ref_pose_inv"][:3, -1]
        ray_d = self._rays(view["ref_pose_inv"], view["ray_o"])
        sample.update({k: v.contiguous()[None].to(self.device) for k, v in view.items()})
        sample["ray_d"] = ray_d[None]
        sample["ref_img"] = self.all_images[render_idx][None]
        return sample


class DtuScan:
    """See the module text.  ``len()`` = ``n_views``; ``scan[i]`` is the batch of render view ``i`` (tensors on ``device``)."""

    def __init__(self, root_dir, scan_id, n_views=3, img_wh=(800, 640), original_img_wh=(1600, 1200), clip_wh=(0, 0), near=425,
                 far=900, set=0, test_view_pair=None, ndepths=192, device="cuda"):
        self.root_dir, self.scan_id, self.n_views, self.device = str(root_dir), scan_id, int(n_views), torch.device(device)
        view_list = test_view_pair if set == 0 else SET1_VIEWS
        if view_list is None or len(view_list) < self.n_views or self.n_views < 1:
            raise ValueError(f"DtuScan: {self.n_views} views asked of the view list {view_list!r}")
        self.idx = list(view_list[:self.n_views])
        data_dir = os.path.join(self.root_dir, scan_id) if scan_id is not None else self.root_dir
        img_wh, clip_wh = [int(v) for v in img_wh], [int(v) for v in clip_wh]
        if len(clip_wh) == 2:
            clip_wh = clip_wh + clip_wh
        img_W, img_H = img_wh[0] - clip_wh[0] - clip_wh[2], img_wh[1] - clip_wh[1] - clip_wh[3]
        if img_W < 2 or img_H < 2:
            raise ValueError(f"DtuScan: clip {clip_wh} leaves {img_H}x{img_W} of the image (at least 2x2 is needed)")
        world_mats = []
        for vid in self.idx:           # depth_min / depth_interval: the last file's
            P, depth_min, depth_interval = read_cam_file(os.path.join(self.root_dir, "cameras/{:0>8}_cam.txt".format(vid)))
            world_mats.append(P)
        raw = [imread_rgb(os.path.join(data_dir, "image/{:0>6}.png".format(vid))) for vid in self.idx]
        if any(r.shape != raw[0].shape for r in raw):
            raise ValueError(f"DtuScan: the images of {data_dir} differ in size")
        self.group = ViewGroup(world_mats, raw, None, [[int(v) for v in original_img_wh]] * self.n_views, img_wh, clip_wh,
                               np.stack([np.array([near, far]) for _ in self.idx]), OFFSET_DIST, depth_min, depth_interval, ndepths,
                               device, cameras.homo_pixels(img_H, img_W))
        g = self.group                 # what the commands and tests read from a scan
        self.img_wh, self.img_W, self.img_H, self.homo_pixel, self.scale_factor = g.img_wh, g.img_W, g.img_H, g.homo_pixel, g.scale_factor
        self.depth_min, self.depth_interval = g.depth_min, g.depth_interval
        self.all_w2cs_original, self.all_render_w2cs_original = g.all_w2cs_original, g.all_render_w2cs_original

    def __len__(self):
        return self.n_views

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __getitem__(self, idx):
        if not -self.n_views <= idx < self.n_views:
            raise IndexError(idx)
        render_idx = idx % self.n_views
        sample = self.group.batch(render_idx)
        sample["meta"] = ["%s-%s-%08d" % (self.root_dir.split("/")[-1], self.scan_id, render_idx)]
        return sample
