"""A DTU test scan as the batches the model reads: the reference's `DtuFitSparse` (code1/dataset/dtu_test_sparse.py:75-436)
with `load_K_Rt_from_P` (:51-72) and `get_boundingbox` / `get_view_frustum` (code1/dataset/scene_transform.py:14-107),
without OpenCV, torchvision or a `DataLoader`.

    scan = DtuScan(test_dir, "scan24", n_views=3, test_view_pair=[23, 24, 33], device="cuda:0")
    for batch in scan:                      # one batch per render view, in the collated batch-of-one form
        net.extract_geometry(batch, out_dir=...)

Who computes what:

  host    every 4x4: the camera files, the decomposition, inverses, the bounding box, the scaled cameras, the poses -- the
          same numpy / CPU-torch calls in the reference's order and dtypes (the reference runs them on the CPU as well), so
          these entries equal the reference's bit for bit (tests/golden/dtu_scan_small.npz went through its own code);
  device  everything per pixel: the images (`ops.image_resize_u8`) and the two ray tables (`ops.pixel_rays`).  With
          ``device="cpu"`` the host forms below (`image_planes_host`, `pixel_rays_host`) stand in.

Restated, not compared (no OpenCV was at hand; the rule written here is the rule):

  `decompose_projection_matrix`  cv2.decomposeProjectionMatrix as far as the loader uses it: an RQ factorisation of P[:, :3] in
          float64 with a positive diagonal in K, the camera centre -M^-1 p4 as a homogeneous column with w = 1, all rounded to
          P's dtype.  (OpenCV takes the centre from an SVD and scales it to unit length: the loader divides by w either way.)
  `resize_u8`  cv2.resize for 8-bit images with the default INTER_LINEAR: its fixed-point arithmetic as include/ufr.h
          (ufr_image_resize_u8) states it, the 2x2 box mean when both factors are exactly 2.

Quirks of the reference that are kept (the goldens have them): `depth_min` and `depth_interval` (x 1.06) are those of the LAST
camera file read; `depth_values_org_scale` is `np.arange(min, max, interval, float32)` whatever its length; the render camera
is the source camera moved 25 mm along its own x axis; `proj_matrices` holds the UNSCALED `all_w2cs` and leaves [1, 3, 3] zero;
the ray tables are computed in float64 and cast at the end; scan-level tensors are shared between the batches of one scan.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .clean_mesh import SET1_VIEWS

OFFSET_DIST = 25      # mm, dtu_test_sparse.py:88


# ------------------------------------------------------------------ OpenCV, restated
def decompose_projection_matrix(P):
    """(K (3,3), R (3,3), centre (4,1)) of a 3x4 projection matrix P = K [R | -R c]: see the module text."""
    P = np.asarray(P)
    M = P[:, :3].astype(np.float64)
    q, r = np.linalg.qr(np.flipud(M).T)            # RQ through the QR of the reversed, transposed matrix
    K = np.flipud(r.T)[:, ::-1]
    R = q.T[::-1, :]
    sign = np.where(np.diag(K) < 0, -1.0, 1.0)
    K = K * sign[None, :]
    R = R * sign[:, None]
    c = -np.linalg.solve(M, P[:, 3].astype(np.float64))
    centre = np.concatenate([c, [1.0]])[:, None]
    dt = P.dtype if P.dtype.kind == "f" else np.float64
    return K.astype(dt), R.astype(dt), centre.astype(dt)


def _taps(n_dst: int, n_src: int, along_x: bool):
    d = np.arange(n_dst, dtype=np.float64)
    scale = np.float64(n_src) / np.float64(n_dst)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    if along_x:                                    # a tap outside the row: the edge pixel with weight 1
        lo, hi = s < 0, s >= n_src - 1
        s[lo], f[lo] = 0, 0
        s[hi], f[hi] = n_src - 1, 0
    s0 = np.clip(s, 0, n_src - 1)
    s1 = np.clip(s + 1, 0, n_src - 1)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    w1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s0, s1, w0, w1


def resize_u8(image, size):
    """cv2.resize(image, (W, H)) for uint8 images (..., Hs, Ws, C): see the module text."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim < 3:
        raise ValueError(f"resize_u8: expected a uint8 array (..., H, W, C), got {img.dtype} {img.shape}")
    W, H = int(size[0]), int(size[1])
    Hs, Ws = img.shape[-3], img.shape[-2]
    if W < 1 or H < 1 or Hs < 1 or Ws < 1:
        raise ValueError(f"resize_u8: {Hs}x{Ws} -> {H}x{W}")
    v = img.astype(np.int32)
    if Hs == 2 * H and Ws == 2 * W:
        out = (v[..., 0::2, 0::2, :] + v[..., 0::2, 1::2, :] + v[..., 1::2, 0::2, :] + v[..., 1::2, 1::2, :] + 2) >> 2
        return out.astype(np.uint8)
    x0, x1, a0, a1 = _taps(W, Ws, True)
    y0, y1, b0, b1 = _taps(H, Hs, False)
    rows = v[..., :, x0, :] * a0[:, None] + v[..., :, x1, :] * a1[:, None]            # (..., Hs, W, C) int32
    r0, r1 = rows[..., y0, :, :], rows[..., y1, :, :]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def imread_rgb(path):
    """An 8-bit image file as (H, W, 3) uint8 RGB (cv2.imread gives the same bytes in BGR order)."""
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


# ------------------------------------------------------------------ the host forms of the two kernels
def image_planes_host(images, H: int, W: int, clip=(0, 0, 0, 0)):
    """ufr_image_resize_u8 on the host: (n,Hs,Ws,3) uint8 -> (n,3,Ho,Wo) float32 array, value = float32(double(v) / 255)."""
    images = np.asarray(images)
    H, W = int(H), int(W)
    left, top, right, bottom = (int(c) for c in clip)
    if images.ndim != 4 or images.shape[3] != 3 or min(left, top, right, bottom) < 0 or H - top - bottom < 1 or W - left - right < 1:
        raise ValueError(f"image_planes_host: images {images.shape}, {H}x{W}, clip {tuple(clip)}")
    small = resize_u8(images, (W, H)) / 255.
    small = small[:, top:H - bottom, left:W - right]
    return np.ascontiguousarray(np.transpose(small, (0, 3, 1, 2))).astype(np.float32)


def image_mask_planes_host(images, masks, H: int, W: int, clip=(0, 0, 0, 0)):
    """ufr_image_resize_mask_u8 on the host, in the reference's calls (general_fit.py:174-180): colour (n,Hs,Ws,3) and mask
    (n,Hs,Ws) uint8 each through `resize_u8`, value = float32((v / 255) * (m / 254)) with the product taken in float64."""
    images, masks = np.asarray(images), np.asarray(masks)
    H, W = int(H), int(W)
    left, top, right, bottom = (int(c) for c in clip)
    if images.ndim != 4 or images.shape[3] != 3 or masks.shape != images.shape[:3] or masks.dtype != np.uint8 \
            or min(left, top, right, bottom) < 0 or H - top - bottom < 1 or W - left - right < 1:
        raise ValueError(f"image_mask_planes_host: images {images.shape}, masks {masks.dtype} {masks.shape}, {H}x{W}, clip {tuple(clip)}")
    small = resize_u8(images, (W, H)) / 255.
    small = small * (resize_u8(masks[..., None], (W, H)) / 254.)
    small = small[:, top:H - bottom, left:W - right]
    return np.ascontiguousarray(np.transpose(small, (0, 3, 1, 2))).astype(np.float32)


def homo_pixels(H: int, W: int):
    """dtu_test_sparse.py:171-176: the (4, H*W) float64 table of normalised pixel coordinates (x, y, 1, 1)."""
    h_line = (np.linspace(0, H - 1, H)) * 2 / (H - 1) - 1
    w_line = (np.linspace(0, W - 1, W)) * 2 / (W - 1) - 1
    h_mesh, w_mesh = np.meshgrid(h_line, w_line, indexing="ij")
    w_flat, h_flat = w_mesh.reshape(-1), h_mesh.reshape(-1)
    return np.stack([w_flat, h_flat, np.ones(len(h_flat)), np.ones(len(h_flat))])


def pixel_rays_host(m_inv, H: int, W: int, origin=None, homo_pixel=None):
    """ufr_pixel_rays on the host, in the reference's own calls (dtu_test_sparse.py:423-429): the float32 matrix times the
    float64 table in numpy, minus the origin, over torch.norm, cast to float32.  Returns a (3, H*W) CPU tensor."""
    if int(H) < 2 or int(W) < 2:
        raise ValueError(f"pixel_rays_host: image {H}x{W} (H and W must be >= 2)")
    m = torch.as_tensor(m_inv, dtype=torch.float32)
    hp = homo_pixels(int(H), int(W)) if homo_pixel is None else homo_pixel
    v = torch.from_numpy(np.matmul(m.numpy(), hp))[:3]          # what `tensor @ ndarray` evaluates
    if origin is not None:
        v = v - torch.as_tensor(origin, dtype=torch.float32)[:, None]
    return (v / torch.norm(v, dim=0)).float()


# ------------------------------------------------------------------ the reference's camera arithmetic, call for call
def load_K_Rt_from_P(P):
    """dtu_test_sparse.py:51-72."""
    out = decompose_projection_matrix(P)
    K, R, t = out[0], out[1], out[2]
    K = K / K[2, 2]
    intrinsics = np.eye(4)
    intrinsics[:3, :3] = K
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R.transpose()
    pose[:3, 3] = (t[:3] / t[3])[:, 0]
    return intrinsics, pose


def _rigid_transform(xyz, transform):
    xyz_h = torch.cat([xyz, torch.ones((len(xyz), 1))], dim=1)
    return (transform @ xyz_h.T).T[:, :3]


def get_view_frustum(min_depth, max_depth, size, cam_intr, c2w):
    """scene_transform.py:14-47: the 8 corners of a camera's depth range, in world coordinates."""
    im_h, im_w = int(size[0]), int(size[1])
    depths = [min_depth, min_depth, min_depth, min_depth, max_depth, max_depth, max_depth, max_depth]
    pts = torch.stack([
        (torch.tensor([0, 0, im_w, im_w, 0, 0, im_w, im_w]) - cam_intr[0, 2]) * torch.tensor(depths) / cam_intr[0, 0],
        (torch.tensor([0, im_h, 0, im_h, 0, im_h, 0, im_h]) - cam_intr[1, 2]) * torch.tensor(depths) / cam_intr[1, 1],
        torch.tensor(depths)])
    pts = pts.type(torch.float32)
    return _rigid_transform(pts.T, c2w).T


def get_boundingbox(img_hw, intrinsics, extrinsics, near_fars):
    """scene_transform.py:60-107 for stacked tensors: (centre (3,), radius, bounds (3,2)) of the hull of all view frusta."""
    bnds = torch.zeros((3, 2))
    bnds[:, 0] = np.inf
    bnds[:, 1] = -np.inf
    for i in range(intrinsics.shape[0]):
        c2w = torch.inverse(extrinsics[i])
        pts = get_view_frustum(near_fars[i][0], near_fars[i][1], img_hw, intrinsics[i], c2w)
        bnds[:, 0] = torch.min(bnds[:, 0], torch.min(pts, dim=1)[0])
        bnds[:, 1] = torch.max(bnds[:, 1], torch.max(pts, dim=1)[0])
    center = torch.tensor(((bnds[0, 1] + bnds[0, 0]) / 2, (bnds[1, 1] + bnds[1, 0]) / 2, (bnds[2, 1] + bnds[2, 0]) / 2))
    lengths = bnds[:, 1] - bnds[:, 0]
    max_length, _ = torch.max(lengths, dim=0)
    return center, max_length / 2, bnds


def read_cam_file(filename):
    """dtu_test_sparse.py:185-206: (P = K_4x4 @ E float32, depth_min, depth_interval * 1.06) of a `%08d_cam.txt`."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.fromstring(" ".join(lines[1:5]), dtype=np.float32, sep=" ").reshape((4, 4))
    intrinsics = np.fromstring(" ".join(lines[7:10]), dtype=np.float32, sep=" ").reshape((3, 3))
    intrinsics_ = np.float32(np.diag([1, 1, 1, 1]))
    intrinsics_[:3, :3] = intrinsics
    return intrinsics_ @ extrinsics, float(lines[11].split()[0]), float(lines[11].split()[1]) * 1.06


class DtuScan:
    """See the module text.  ``len()`` = ``n_views``; ``scan[i]`` is the batch of render view ``i`` (tensors on ``device``)."""

    def __init__(self, root_dir, scan_id, n_views=3, img_wh=(800, 640), original_img_wh=(1600, 1200), clip_wh=(0, 0), near=425,
                 far=900, set=0, test_view_pair=None, ndepths=192, device="cuda"):
        self.root_dir, self.scan_id, self.n_views, self.ndepths = str(root_dir), scan_id, int(n_views), ndepths
        self.device = torch.device(device)
        view_list = test_view_pair if set == 0 else SET1_VIEWS
        if view_list is None or len(view_list) < self.n_views or self.n_views < 1:
            raise ValueError(f"DtuScan: {self.n_views} views asked of the view list {view_list!r}")
        self.idx = list(view_list[:self.n_views])
        self.data_dir = os.path.join(self.root_dir, scan_id) if scan_id is not None else self.root_dir
        img_wh, clip_wh = [int(v) for v in img_wh], [int(v) for v in clip_wh]
        if len(clip_wh) == 2:
            clip_wh = clip_wh + clip_wh
        self.clip_wh, self.original_img_wh = clip_wh, [int(v) for v in original_img_wh]

        self.world_mats_np, self.images_list = [], []
        for vid in self.idx:           # depth_min / depth_interval: the last file's
            P, self.depth_min, self.depth_interval = read_cam_file(os.path.join(self.root_dir, "cameras/{:0>8}_cam.txt".format(vid)))
            self.world_mats_np.append(P)
            self.images_list.append(os.path.join(self.data_dir, "image/{:0>6}.png".format(vid)))
        self.raw_near_fars = np.stack([np.array([near, far]) for _ in self.images_list])
        self.ref_w2c = np.linalg.inv(load_K_Rt_from_P(self.world_mats_np[0][:3, :4])[1])

        self._load_scene(img_wh)
        self.img_W, self.img_H = self.img_wh
        if self.img_W < 2 or self.img_H < 2:
            raise ValueError(f"DtuScan: clip {clip_wh} leaves {self.img_H}x{self.img_W} of the image (at least 2x2 is needed)")
        # dtu_test_sparse.py:301-308
        center, radius, _ = get_boundingbox([self.img_H, self.img_W], self.all_intrinsics, self.all_w2cs, self.raw_near_fars)
        radius = radius * 1.1
        scale_mat = np.diag([radius, radius, radius, 1.0])
        scale_mat[:3, 3] = center.cpu().numpy()
        self.scale_mat = scale_mat.astype(np.float32)
        self.scale_factor = 1. / radius.cpu().numpy()
        self._scale_cam_info()
        self.homo_pixel = homo_pixels(self.img_H, self.img_W)
        self._shared = None

    # ---- dtu_test_sparse.py:247-298
    def _load_scene(self, img_wh):
        clip = self.clip_wh
        scale_x = img_wh[0] / self.original_img_wh[0]
        scale_y = img_wh[1] / self.original_img_wh[1]
        raw = [imread_rgb(p) for p in self.images_list]
        if any(r.shape != raw[0].shape for r in raw):
            raise ValueError(f"DtuScan: the images of {self.data_dir} differ in size")
        raw = np.stack(raw)
        if self.device.type == "cuda":
            from . import ops

            with torch.cuda.device(self.device):
                self.all_images = ops.image_resize_u8(torch.from_numpy(raw).to(self.device), img_wh[1], img_wh[0], clip)
        else:
            self.all_images = torch.from_numpy(image_planes_host(raw, img_wh[1], img_wh[0], clip)).to(self.device)
        intr, w2cs, render_w2cs, w2cs_org, render_w2cs_org = [], [], [], [], []
        for P in self.world_mats_np:
            intrinsics, c2w = load_K_Rt_from_P(P[:3, :4])
            w2c = np.linalg.inv(c2w)
            render_c2w = c2w.copy()
            render_c2w[:3, 3] += render_c2w[:3, 0] * OFFSET_DIST
            render_w2c = np.linalg.inv(render_c2w)
            intrinsics[:1] *= scale_x
            intrinsics[1:2] *= scale_y
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
        self.img_wh = [img_wh[0] - clip[0] - clip[2], img_wh[1] - clip[1] - clip[3]]

    # ---- dtu_test_sparse.py:311-376
    def _scale_cam_info(self):
        w2cs, c2ws, near_fars, render_w2cs, render_c2ws, proj = [], [], [], [], [], []
        for idx in range(self.n_views):
            intrinsics = self.all_intrinsics[idx]
            P = np.matmul((intrinsics @ self.all_w2cs[idx]).numpy(), self.scale_mat)[:3, :4]     # `tensor @ ndarray`
            c2w = load_K_Rt_from_P(P)[1]
            w2cs.append(np.linalg.inv(c2w))
            c2ws.append(c2w)
            camera_o = c2w[:3, 3]
            dist = np.sqrt(np.sum(camera_o ** 2))
            near_fars.append([0.95 * (dist - 1), 1.05 * (dist + 1)])
            proj_mat = np.zeros(shape=(2, 4, 4), dtype=np.float32)
            intrinsic_cp = self.all_intrinsics[idx].clone()[:3, :3]
            intrinsic_cp[:2] /= 4
            proj_mat[0, :4, :4] = self.all_w2cs[idx].numpy()
            proj_mat[1, :3, :3] = intrinsic_cp.numpy()
            proj.append(proj_mat)
            P = np.matmul((intrinsics @ self.all_render_w2cs[idx]).numpy(), self.scale_mat)[:3, :4]
            c2w = load_K_Rt_from_P(P)[1]
            render_w2cs.append(np.linalg.inv(c2w))
            render_c2ws.append(c2w)
        f32 = lambda xs: torch.from_numpy(np.float32(np.stack(xs)))  # noqa: E731
        self.scaled_intrinsics = self.all_intrinsics.clone()
        self.scaled_w2cs, self.scaled_c2ws, self.scaled_near_fars = f32(w2cs), f32(c2ws), f32(near_fars)
        self.scaled_render_w2cs, self.scaled_render_c2ws = f32(render_w2cs), f32(render_c2ws)
        stage1 = np.stack(proj)
        stage2, stage3 = stage1.copy(), stage1.copy()
        stage2[:, 1, :2, :] = stage1[:, 1, :2, :] * 2
        stage3[:, 1, :2, :] = stage1[:, 1, :2, :] * 4
        self.proj_matrices_ms = {"stage1": stage1, "stage2": stage2, "stage3": stage3}

    def __len__(self):
        return self.n_views

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def _rays(self, m_inv, origin):
        if self.device.type == "cuda":
            from . import ops

            return ops.pixel_rays(m_inv.numpy(), self.img_H, self.img_W, None if origin is None else origin.numpy(), self.device)
        return pixel_rays_host(m_inv, self.img_H, self.img_W, origin, self.homo_pixel)

    def _scan_level(self):
        """What every render view of the scan shares (dtu_test_sparse.py:387-419 without the view's own entries)."""
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
            intrinsics_pad = torch.eye(4).expand(V, 4, 4).clone()
            intrinsics_pad[:, :3, :3] = s["intrinsics"]
            normalize_matrix = torch.tensor([[1 / ((self.img_W - 1) / 2), 0, -1, 0], [0, 1 / ((self.img_H - 1) / 2), -1, 0],
                                             [0, 0, 1, 0], [0, 0, 0, 1]])
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

    def __getitem__(self, idx):
        if not -self.n_views <= idx < self.n_views:
            raise IndexError(idx)
        render_idx = idx % self.n_views
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
        sample["meta"] = ["%s-%s-%08d" % (self.root_dir.split("/")[-1], self.scan_id, render_idx)]
        return sample
