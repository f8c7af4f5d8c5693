"""The host camera arithmetic the loaders share (`dtu_scan`, `dtu_train`, `general_scan`, `clean_mesh`, `depth_fusion`): the two
text files of an MVSNet-style scene, and the reference's 4x4 work in its own numpy / CPU-torch calls, order and dtypes
(code1/dataset/dtu_test_sparse.py, dtu_train.py, general_fit.py and scene_transform.py write it out once each).  numpy and CPU
torch only: no picture is read here and no kernel is called (`host_forms` has both).

Restated, not compared (no OpenCV was at hand; the rule written here is the rule):

  `decompose_projection_matrix`  cv2.decomposeProjectionMatrix as far as the loaders use it: an RQ factorisation of P[:, :3] in
          float64 with a positive diagonal in K, the camera centre -M^-1 p4 as a homogeneous column with w = 1, all rounded to
          P's dtype.  (OpenCV takes the centre from an SVD and scales it to unit length: the loaders divide by w either way.)

How P is formed differs per loader (a torch product then a numpy one in `dtu_scan.ViewGroup`, numpy float32 in `DtuTrain`) and
stays with the caller, as do the dtypes of the near / far values that go into `get_boundingbox`: the goldens pin those bits.
"""
from __future__ import annotations

import numpy as np
import torch


# ------------------------------------------------------------------ the two text files
def read_cam_file(filename):
    """(K 3x3 float32, E 4x4 float32, the depth line's tokens as floats) of a `%08d_cam.txt`, parsed as the reference's
    `read_cam_file`s parse it.  The tokens are depth_min, depth_interval and whatever follows (the sample count, depth_max)."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.fromstring(" ".join(lines[1:5]), dtype=np.float32, sep=" ").reshape((4, 4))
    intrinsics = np.fromstring(" ".join(lines[7:10]), dtype=np.float32, sep=" ").reshape((3, 3))
    return intrinsics, extrinsics, [float(t) for t in lines[11].split()]


def read_pair_file(path):
    """[(ref view, [source views])] of an MVSNet pair file, every entry kept (an entry without sources as well)."""
    entries = []
    with open(path) as f:
        for _ in range(int(f.readline())):
            ref_view = int(f.readline().rstrip())
            entries.append((ref_view, [int(x) for x in f.readline().rstrip().split()[1::2]]))
    return entries


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


def scale_matrix(center, radius):
    """dtu_test_sparse.py:301-308 / cal_scale_mat (dtu_train.py:299-307): (scale_mat 4x4 float32, scale_factor) of the sphere
    `get_boundingbox` gives, its radius widened by 1.1."""
    radius = radius * 1.1
    scale_mat = np.diag([radius, radius, radius, 1.0])
    scale_mat[:3, 3] = center.cpu().numpy()
    return scale_mat.astype(np.float32), 1. / radius.cpu().numpy()


def scaled_camera(P):
    """(w2c, c2w, [near, far]) of the 3x4 projection ``P`` = K @ w2c @ scale_mat: the camera in units of the bounding sphere,
    near / far from its distance to the origin (dtu_test_sparse.py:318-329)."""
    c2w = load_K_Rt_from_P(P)[1]
    dist = np.sqrt(np.sum(c2w[:3, 3] ** 2))
    return np.linalg.inv(c2w), c2w, [0.95 * (dist - 1), 1.05 * (dist + 1)]


def proj_matrices_ms(extrinsics, intrinsics):
    """The `proj_matrices` of the cascade (dtu_test_sparse.py:331-376): for (n,4,4) extrinsics and (n,>=3,>=3) float32
    intrinsics of the full-size picture, {"stage1" .. "stage3": (n,2,4,4) float32} -- [:, 0] the extrinsics, [:, 1, :3, :3] the
    intrinsics at a quarter, a half and the whole of the size; [:, 1, 3, 3] stays zero as in the reference."""
    stage1 = np.zeros((len(extrinsics), 2, 4, 4), dtype=np.float32)
    stage1[:, 0] = np.asarray(extrinsics)
    stage1[:, 1, :3, :3] = np.asarray(intrinsics)[:, :3, :3]
    stage1[:, 1, :2] /= 4
    stage2, stage3 = stage1.copy(), stage1.copy()
    stage2[:, 1, :2, :] = stage1[:, 1, :2, :] * 2
    stage3[:, 1, :2, :] = stage1[:, 1, :2, :] * 4
    return {"stage1": stage1, "stage2": stage2, "stage3": stage3}


def normalize_matrix(H: int, W: int):
    """Pixel coordinates -> [-1, 1]^2, as a 4x4 float32 tensor (dtu_test_sparse.py:402-403)."""
    return torch.tensor([[1 / ((W - 1) / 2), 0, -1, 0], [0, 1 / ((H - 1) / 2), -1, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def pad_intrinsics(intrinsics):
    """(V,3,3) float32 tensor -> (V,4,4): each matrix in the corner of an identity."""
    pad = torch.eye(4).expand(len(intrinsics), 4, 4).clone()
    pad[:, :3, :3] = intrinsics
    return pad


def homo_pixels(H: int, W: int):
    """dtu_test_sparse.py:171-176: the (4, H*W) float64 table of normalised pixel coordinates (x, y, 1, 1)."""
    h_line = (np.linspace(0, H - 1, H)) * 2 / (H - 1) - 1
    w_line = (np.linspace(0, W - 1, W)) * 2 / (W - 1) - 1
    h_mesh, w_mesh = np.meshgrid(h_line, w_line, indexing="ij")
    w_flat, h_flat = w_mesh.reshape(-1), h_mesh.reshape(-1)
    return np.stack([w_flat, h_flat, np.ones(len(h_flat)), np.ones(len(h_flat))])
