"""Host side of TSDF fusion: a mirror of the reference's ``TSDFVolume`` (tsdf_fusion.py:20-357) whose ``integrate``
runs the HIP kernel of csrc/tsdf.hip instead of a pycuda-compiled CUDA string.  Same constructor arguments, same
attribute names, same ``integrate`` / ``get_volume`` signatures; the volumes live in HBM.  No CPU fallback: without a
GPU or libufr.so the constructor raises ``UfrError``.  ``get_mesh`` / ``get_point_cloud`` run marching cubes on the device
(csrc/mcubes.hip); ``meshwrite`` / ``pcwrite`` / ``save_tsdf`` and ``python -m uforecon_amd.tsdf`` mirror the rest of
tsdf_fusion.py (:384-534).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .ops import UfrError, _stream


def rigid_transform(xyz, transform):
    """tsdf_fusion.py:359-364"""
    xyz_h = np.hstack([xyz, np.ones((len(xyz), 1), dtype=np.float32)])
    return np.dot(transform, xyz_h.T).T[:, :3]


def get_view_frustum(depth_im, cam_intr, cam_pose):
    """Corners of the camera frustum out to the largest depth, world coordinates (tsdf_fusion.py:367-381)."""
    im_h, im_w = depth_im.shape
    max_depth = np.max(depth_im)
    far = np.array([0, max_depth, max_depth, max_depth, max_depth])
    pts = np.array([(np.array([0, 0, 0, im_w, im_w]) - cam_intr[0, 2]) * far / cam_intr[0, 0],
                    (np.array([0, 0, im_h, 0, im_h]) - cam_intr[1, 2]) * far / cam_intr[1, 1], far])
    return rigid_transform(pts.T, cam_pose).T


class TSDFVolume:
    """Volumetric TSDF fusion of depth maps (tsdf_fusion.py:20).  ``use_gpu`` is accepted for signature
    compatibility; there is only the GPU path.  ``integrate_color=False`` is the reference's behaviour (its kernel
    returns before the colour block, tsdf_fusion.py:139): the colour volume stays zero."""

    def __init__(self, vol_bnds, voxel_size, use_gpu=True, margin=5, device="cuda:0", integrate_color=False):
        if not torch.cuda.is_available():
            raise UfrError("TSDFVolume needs a GPU: there is no CPU fallback")
        self._lib = _lib.load()
        vol_bnds = np.asarray(vol_bnds, dtype=np.float64)
        assert vol_bnds.shape == (3, 2), "[!] `vol_bnds` should be of shape (3, 2)."
        self._vol_bnds = vol_bnds
        self._voxel_size = float(voxel_size)
        self._trunc_margin = margin * self._voxel_size
        self._color_const = 256 * 256
        self._vol_dim = np.round((self._vol_bnds[:, 1] - self._vol_bnds[:, 0]) / self._voxel_size).copy(order="C").astype(int)
        self._vol_bnds[:, 1] = self._vol_bnds[:, 0] + self._vol_dim * self._voxel_size
        self._vol_origin = self._vol_bnds[:, 0].copy(order="C").astype(np.float32)
        self.device = torch.device(device)
        self.integrate_color = bool(integrate_color)
        dim = tuple(int(d) for d in self._vol_dim)
        self._tsdf_vol_gpu = torch.ones(dim, dtype=torch.float32, device=self.device)
        self._weight_vol_gpu = torch.zeros(dim, dtype=torch.float32, device=self.device)
        self._color_vol_gpu = torch.zeros(dim, dtype=torch.float32, device=self.device)
        self.gpu_mode = True

    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1.0):
        """color_im (H,W,3) or None, depth_im (H,W), cam_intr 3x3, cam_pose 4x4 camera-to-world (tsdf_fusion.py:220-265).
        Images may be numpy arrays (copied to the device) or device tensors."""
        dev = self.device
        depth = torch.as_tensor(np.asarray(depth_im, np.float32) if not torch.is_tensor(depth_im) else depth_im,
                                dtype=torch.float32).to(dev).contiguous()
        im_h, im_w = depth.shape
        folded = None
        if color_im is not None and self.integrate_color:
            c = torch.as_tensor(np.asarray(color_im, np.float32) if not torch.is_tensor(color_im) else color_im,
                                dtype=torch.float32).to(dev)
            folded = torch.floor(c[..., 2] * float(self._color_const) + c[..., 1] * 256.0 + c[..., 0]).contiguous()   # :235-238
        f32p = C.POINTER(C.c_float)
        dim = (C.c_int32 * 3)(*[int(d) for d in self._vol_dim])
        org = np.ascontiguousarray(self._vol_origin, np.float32)
        K = np.ascontiguousarray(np.asarray(cam_intr, np.float32).reshape(-1)[:9])
        P = np.ascontiguousarray(np.asarray(cam_pose, np.float32).reshape(-1)[:16])
        _lib.check(self._lib.ufr_tsdf_integrate(
            self._tsdf_vol_gpu.data_ptr(), self._weight_vol_gpu.data_ptr(), self._color_vol_gpu.data_ptr(), dim,
            org.ctypes.data_as(f32p), self._voxel_size, self._trunc_margin, K.ctypes.data_as(f32p), P.ctypes.data_as(f32p),
            depth.data_ptr(), folded.data_ptr() if folded is not None else None, im_h, im_w, float(obs_weight),
            1 if folded is not None else 0, _stream()), "ufr_tsdf_integrate")

    def get_volume(self):
        """(tsdf, color, weight) as numpy arrays (tsdf_fusion.py:312-317)."""
        return (self._tsdf_vol_gpu.cpu().numpy(), self._color_vol_gpu.cpu().numpy(), self._weight_vol_gpu.cpu().numpy())

    def _mesh_device(self):
        """Marching cubes + vertex colours on the device; only the mesh crosses to the host."""
        from .ops import marching_cubes

        verts, faces, norms = marching_cubes(self._tsdf_vol_gpu, 0.0)
        ind = torch.round(verts).long()                        # half to even, as np.round
        rgb = self._color_vol_gpu[ind[:, 0], ind[:, 1], ind[:, 2]]
        c = float(self._color_const)
        b = torch.floor(rgb / c)
        g = torch.floor((rgb - b * c) / 256)
        r = rgb - b * c - g * 256
        colors = torch.floor(torch.stack([r, g, b], dim=1)).to(torch.uint8)
        origin = torch.from_numpy(self._vol_origin).to(self.device)
        verts = verts * self._voxel_size + origin               # voxel grid -> world, fp32 as in the reference
        return verts.cpu().numpy(), faces.cpu().numpy(), norms.cpu().numpy(), colors.cpu().numpy()

    def get_mesh(self, method="gpu"):
        """Marching cubes over the fused volume (tsdf_fusion.py:340-357): (verts (V,3) world fp32, faces (F,3) int32,
        norms (V,3) fp32, colors (V,3) uint8 r,g,b).  ``method="gpu"``: the HIP kernel (ops.marching_cubes), the volumes
        stay on the device; an empty mesh when the TSDF has no zero crossing.  ``method="skimage"``: the reference's
        scikit-image call on a host copy of the volumes (needs scikit-image; Lewiner's ambiguity resolution, so
        triangles inside ambiguous cubes may differ from the kernel's)."""
        if method == "gpu":
            return self._mesh_device()
        if method != "skimage":
            raise UfrError(f"get_mesh: unknown method {method!r} (gpu, skimage)")
        try:
            from skimage import measure
        except ImportError as e:  # pragma: no cover
            raise UfrError("get_mesh(method='skimage') needs scikit-image") from e
        tsdf_vol, color_vol, _ = self.get_volume()
        mc = getattr(measure, "marching_cubes_lewiner", None) or measure.marching_cubes
        verts, faces, norms, _ = mc(tsdf_vol, level=0)
        verts_ind = np.round(verts).astype(int)
        verts = verts * self._voxel_size + self._vol_origin
        rgb = color_vol[verts_ind[:, 0], verts_ind[:, 1], verts_ind[:, 2]]
        b = np.floor(rgb / self._color_const)
        g = np.floor((rgb - b * self._color_const) / 256)
        r = rgb - b * self._color_const - g * 256
        return verts, faces, norms, np.floor(np.asarray([r, g, b])).T.astype(np.uint8)

    def get_point_cloud(self, method="gpu"):
        """The mesh's vertices with their colours, (V,6) = [x y z r g b] (tsdf_fusion.py:319-338)."""
        verts, _, _, colors = self.get_mesh(method)
        return np.hstack([verts, colors])


def _ply_lines(fmt_cols):
    """Lines of an ASCII PLY body, one per row: each column formatted with its printf format, joined by spaces."""
    line = None
    for fmt, col in fmt_cols:
        s = np.char.mod(fmt, col)
        line = s if line is None else np.char.add(np.char.add(line, " "), s)
    return line


def _write_ply(filename, header, body):
    with open(filename, "w") as f:
        f.write("".join(h + "\n" for h in header))
        if body is not None and len(body):
            f.write("\n".join(body.tolist()))
            f.write("\n")


def meshwrite(filename, verts, faces, norms, colors):
    """A mesh as an ASCII .ply file, the reference's layout (tsdf_fusion.py:384-424): per vertex "%f %f %f %f %f %f %d
    %d %d" (position, normal, r g b), per face "3 %d %d %d".  Built with vectorised numpy formatting."""
    verts, faces, norms, colors = (np.asarray(a) for a in (verts, faces, norms, colors))
    header = ["ply", "format ascii 1.0", "element vertex %d" % verts.shape[0], "property float x", "property float y",
              "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
              "property uchar green", "property uchar blue", "element face %d" % faces.shape[0],
              "property list uchar int vertex_index", "end_header"]
    vl = _ply_lines([("%f", verts[:, 0]), ("%f", verts[:, 1]), ("%f", verts[:, 2]), ("%f", norms[:, 0]),
                     ("%f", norms[:, 1]), ("%f", norms[:, 2]), ("%d", colors[:, 0]), ("%d", colors[:, 1]),
                     ("%d", colors[:, 2])]) if len(verts) else np.empty(0, str)
    fl = np.char.add("3 ", _ply_lines([("%d", faces[:, 0]), ("%d", faces[:, 1]), ("%d", faces[:, 2])])) \
        if len(faces) else np.empty(0, str)
    _write_ply(filename, header, np.concatenate([vl, fl]))


def pcwrite(filename, xyzrgb):
    """A point cloud as an ASCII .ply file, the reference's layout (tsdf_fusion.py:427-444): "%f %f %f %d %d %d"."""
    xyzrgb = np.asarray(xyzrgb)
    xyz = xyzrgb[:, :3]
    rgb = xyzrgb[:, 3:].astype(np.uint8)
    header = ["ply", "format ascii 1.0", "element vertex %d" % xyz.shape[0], "property float x", "property float y",
              "property float z", "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    body = _ply_lines([("%f", xyz[:, 0]), ("%f", xyz[:, 1]), ("%f", xyz[:, 2]), ("%d", rgb[:, 0]), ("%d", rgb[:, 1]),
                       ("%d", rgb[:, 2])]) if len(xyz) else None
    _write_ply(filename, header, body)


def fuse_depth_maps(depths, intrinsics, extrinsics, voxel_size=1.5, margin=3, colors=None, integrate_color=False):
    """The loop of the reference's save_tsdf (tsdf_fusion.py:459-499) over in-memory frames: bounds = hull of the view
    frusta (starting from the origin), then one `integrate` per view with cam_pose = inverse(extrinsic)."""
    poses = [np.linalg.inv(E) for E in extrinsics]
    vol_bnds = np.zeros((3, 2))
    for d, K, P in zip(depths, intrinsics, poses):
        pts = get_view_frustum(np.asarray(d), K, P)
        vol_bnds[:, 0] = np.minimum(vol_bnds[:, 0], np.amin(pts, axis=1))
        vol_bnds[:, 1] = np.maximum(vol_bnds[:, 1], np.amax(pts, axis=1))
    vol = TSDFVolume(vol_bnds, voxel_size=voxel_size, margin=margin, integrate_color=integrate_color)
    for i, (d, K, P) in enumerate(zip(depths, intrinsics, poses)):
        vol.integrate(None if colors is None else colors[i], d, K, P, obs_weight=1.0)
    return vol


def read_img(filename):
    """tsdf_fusion.py:13-17: an 8-bit image as fp32 in [0, 1]."""
    from PIL import Image

    return np.array(Image.open(filename), dtype=np.float32) / 255.


def save_tsdf(root_dir, scan, n_view=0, test_view=None, voxel_size=1.5, margin=3, integrate_color=False):
    """The reference's save_tsdf (tsdf_fusion.py:447-503) on the files ``model.save_depth_outputs`` writes: fuse
    ``<root_dir>/depth/<scan>/refview<i>.npy`` and write ``<root_dir>/mesh/<scan>.ply`` (meshwrite) and
    ``<root_dir>/pcd/<scan>.ply`` (pcwrite).  Views: ``test_view`` if given, else 0..n_view-1 (missing files skipped),
    else as many as ``<root_dir>/rgb/<scan>`` holds.  Colour images are read only with ``integrate_color`` (the
    reference reads them, but its kernel never integrates colour).  Returns (V, F)."""
    import os

    if test_view is not None:
        views = list(test_view)
    elif n_view > 0:
        views = list(range(n_view))
    else:
        views = list(range(len(os.listdir(os.path.join(root_dir, "rgb", scan)))))
    frames = []
    for i in views:
        path = os.path.join(root_dir, "depth", scan, "refview{}.npy".format(i))
        if test_view is None and not os.path.exists(path):
            continue
        d = np.load(path, allow_pickle=True).item()
        frames.append((i, d["depth"], d["intrinsic"], np.linalg.inv(d["extrinsic"])))
    vol_bnds = np.zeros((3, 2))
    for _, depth_im, cam_intr, cam_pose in frames:
        pts = get_view_frustum(depth_im, cam_intr, cam_pose)
        vol_bnds[:, 0] = np.minimum(vol_bnds[:, 0], np.amin(pts, axis=1))
        vol_bnds[:, 1] = np.maximum(vol_bnds[:, 1], np.amax(pts, axis=1))
    vol = TSDFVolume(vol_bnds, voxel_size=voxel_size, margin=margin, integrate_color=integrate_color)
    for i, depth_im, cam_intr, cam_pose in frames:
        color = read_img(os.path.join(root_dir, "rgb", scan, "refview{}.jpg".format(i))) if integrate_color else None
        vol.integrate(color, depth_im, cam_intr, cam_pose, obs_weight=1.)
    verts, faces, norms, colors = vol.get_mesh()
    os.makedirs(os.path.join(root_dir, "mesh"), exist_ok=True)
    os.makedirs(os.path.join(root_dir, "pcd"), exist_ok=True)
    meshwrite(os.path.join(root_dir, "mesh", "{}.ply".format(scan)), verts, faces, norms, colors)
    pcwrite(os.path.join(root_dir, "pcd", "{}.ply".format(scan)), np.hstack([verts, colors]))   # = get_point_cloud()
    return len(verts), len(faces)


def main(argv=None):
    """``python -m uforecon_amd.tsdf --root_dir DIR ...``: the reference's command line (tsdf_fusion.py:506-534)."""
    import argparse
    import os

    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset", dest="dataset", type=str, default="DTU", help="dataset name")
    parser.add_argument("--root_dir", dest="root_dir", type=str, help="directory of depth maps")
    parser.add_argument("--n_view", dest="n_view", type=int, default=0)
    parser.add_argument("--voxel_size", type=float, default=1.5, help="voxel size")
    parser.add_argument("--margin", default=3, type=int)
    parser.add_argument("--test_view", type=int, nargs="+", default=None)
    parser.add_argument("--test_scan", dest="test_scan", type=str, nargs="+", default=[""])
    parser.add_argument("--integrate_color", action="store_true", help="also fuse the colour images (the reference does not)")
    args = parser.parse_args(argv)
    scans = os.listdir(args.root_dir)
    if args.dataset == "DTU":
        scans = [s for s in scans if s[:4] == "scan"]
    else:
        scans = [s for s in scans if s in args.test_scan]
    print("found scans:", scans)
    for scan in sorted(scans):
        V, F = save_tsdf(args.root_dir, scan, n_view=args.n_view, test_view=args.test_view, voxel_size=args.voxel_size,
                         margin=args.margin, integrate_color=args.integrate_color)
        print(f"{scan}: {V} vertices, {F} faces -> mesh/{scan}.ply, pcd/{scan}.ply")


if __name__ == "__main__":
    main()
