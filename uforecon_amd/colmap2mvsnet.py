"""A COLMAP sparse model as the MVSNet-style scene directory the custom-scene loader reads: the reference's colmap2mvsnet.py,
under its flag names, with the view selection on the GPU.

    python -m uforecon_amd.colmap2mvsnet --dense_folder SCENE [--max_d 0 --interval_scale 1 --theta0 5 --sigma1 1 --sigma2 10]

reads ``SCENE/sparse/0/{cameras,images,points3D}.bin`` and writes ``SCENE/cams/%08d_cam.txt``, ``SCENE/pair.txt`` (where the
reference writes it) and ``SCENE/cams/pair.txt`` (where its loader, and `general_scan.GeneralScan`, read it: that second copy is
ours), and copies ``SCENE/images/<name>`` to ``SCENE/images/%08d.jpg`` and ``SCENE/masks/<name>.png``, where there is one, to
``SCENE/masks/%08d_mask.jpg``.  `convert(...)` is the same in memory.

Who computes what:

  host    everything that is O(observations): the files, the intrinsics by camera model, the extrinsics from `qvec` / `tvec`,
          the depth ranges (the 1 % and 99 % order statistics of the camera-space z of an image's valid observations) and
          `depth_num` (the one-pixel-baseline formula when ``--max_d 0``) -- float64 numpy, the reference's expressions;
  device  the score of every image pair (`ops.view_pair_scores`, csrc/view_select.hip): the all-pairs step for which the
          reference starts one process per CPU.  With ``device="cpu"`` the host form `pair_scores_host` stands in;
  host    the ranking, the reference's own expression on those scores: ``np.argsort(score[i])[::-1][:10]``.

The binary reader is written from COLMAP's public description of the three files (little endian):

  cameras.bin   uint64 n; per camera: int32 id, int32 model, uint64 width, uint64 height, float64 params[PARAMS[model]]
  images.bin    uint64 n; per image: int32 id, float64 qvec[4] (w x y z), float64 tvec[3], int32 camera id, the name and a
                zero byte, uint64 m, then m records (float64 x, float64 y, int64 point id; -1 = no 3-D point)
  points3D.bin  uint64 n; per point: uint64 id, float64 xyz[3], uint8 rgb[3], float64 error, uint64 t, then t records
                (int32 image id, int32 observation index)

Kept from the reference: image ids must be 1 .. N (it indexes ``images[i + 1]``; anything else ends the command with one line,
exit code 2); the text formats (``str()`` of each float64 in the matrices, ``%f`` for the depth line and the pair scores);
a point that image i observed twice counts twice.  Different, on purpose: the `acos` argument is clamped to [-1, 1] (the
reference gets NaN when rounding carries it past 1); ``--test`` does what its help text says and writes nothing (the reference
ignores it); an image without a valid observation is an error that names the image (the reference raises IndexError); with
``--convert_format`` the pictures AND the masks are re-encoded through PIL (the reference re-encodes the pictures through cv2
and forgets the masks) -- those bytes are not comparable with cv2's.

Lens distortion.  `intrinsic_of` keeps fx, fy, cx, cy of a camera and drops its distortion coefficients, as the
reference does: it expects COLMAP's own undistorter to have run.  For a model straight out of COLMAP's mapper (its default camera
is SIMPLE_RADIAL) that is wrong by the distortion, so the command names the model in one line on stderr, and

    python -m uforecon_amd.colmap2mvsnet --dense_folder SCENE --undistort [--undistort_fit inside|keep]

resamples the pictures to pinhole cameras itself (`undistort.undistort_images`; on the device, ufr_image_undistort_u8 of
csrc/undistort.hip, in groups of at most 8 pictures that share a camera).  Per camera the output keeps the source size and
cx, cy; fx' = z fx, fy' = z fy.  ``keep`` is z = 1 and leaves blank pixels where the output looks past the source picture;
``inside`` (the default) is the smallest z in [1, 4] for which every border pixel of the output has a source: 1 if that holds
already, else 40 bisections of that predicate on [1, 4], taking the upper end -- a longer focal length at the same size only
ever crops, so the search evaluates the distortion and never needs its inverse; a camera for which z = 4 does not suffice ends
the command with one line that names it.  ``cams/%08d_cam.txt`` carries K', and `depth_num`'s one-pixel-baseline formula uses
K' too; ``pair.txt`` does not depend on K.  ``images/%08d.jpg`` and ``masks/%08d_mask.jpg`` are written through PIL as JPEG of
quality 95 without chroma subsampling (`JPEG_OPTIONS`); the mask is the undistorted ``masks/<name>.png``, or 255 where there is
none, and 0 wherever an output pixel has no source, so ``GeneralScan --use_mask`` ignores blank pixels.  SIMPLE_PINHOLE and
PINHOLE cameras are copied as without the flag; FOV and THIN_PRISM_FISHEYE end the command with one line.  Without the flag every
written file is what it was before the flag existed.  The rule restates COLMAP's public camera models and was compared with
neither COLMAP nor OpenCV, and no real scene has been run through it.
"""
from __future__ import annotations

import argparse
import os
import shutil
import struct
import sys
from collections import namedtuple

import numpy as np

Camera = namedtuple("Camera", ["id", "model", "width", "height", "params"])
Image = namedtuple("Image", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])
Point3D = namedtuple("Point3D", ["id", "xyz", "rgb", "error", "image_ids", "point2D_idxs"])

# model id -> (name, number of parameters, True when the first parameter is the one focal length f)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3, True), 1: ("PINHOLE", 4, False), 2: ("SIMPLE_RADIAL", 4, True), 3: ("RADIAL", 5, True),
                 4: ("OPENCV", 8, False), 5: ("OPENCV_FISHEYE", 8, False), 6: ("FULL_OPENCV", 12, False), 7: ("FOV", 5, False),
                 8: ("SIMPLE_RADIAL_FISHEYE", 4, True), 9: ("RADIAL_FISHEYE", 5, True), 10: ("THIN_PRISM_FISHEYE", 12, False)}
MODEL_IDS = {name: k for k, (name, _, _) in CAMERA_MODELS.items()}
PINHOLE_MODELS = ("SIMPLE_PINHOLE", "PINHOLE")      # no distortion: --undistort copies their pictures
UNDISTORT_FITS = ("inside", "keep")
JPEG_OPTIONS = {"quality": 95, "subsampling": 0}    # of the files --undistort writes (4:4:4 chroma; PIL's default is 75, 4:2:0)
TOP_VIEWS = 10       # colmap2mvsnet.py:408


class ColmapError(ValueError):
    """what ends the command with one line"""


# ------------------------------------------------------------------ the three files
def read_cameras_bin(path):
    buf = open(path, "rb").read()
    (n,), pos = struct.unpack_from("<Q", buf, 0), 8
    cameras = {}
    for _ in range(n):
        cid, model, width, height = struct.unpack_from("<iiQQ", buf, pos)
        pos += 24
        if model not in CAMERA_MODELS:
            raise ColmapError(f"{path}: camera {cid} has the unknown model id {model}")
        name, n_params, _ = CAMERA_MODELS[model]
        params = np.frombuffer(buf, "<f8", n_params, pos).copy()
        pos += 8 * n_params
        cameras[cid] = Camera(cid, name, width, height, params)
    return cameras


def read_images_bin(path):
    buf = open(path, "rb").read()
    (n,), pos = struct.unpack_from("<Q", buf, 0), 8
    rec = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
    images = {}
    for _ in range(n):
        iid = struct.unpack_from("<i", buf, pos)[0]
        qt = np.frombuffer(buf, "<f8", 7, pos + 4).copy()
        cid = struct.unpack_from("<i", buf, pos + 60)[0]
        pos += 64
        end = buf.index(b"\x00", pos)
        name = buf[pos:end].decode("utf-8")
        (m,), pos = struct.unpack_from("<Q", buf, end + 1), end + 9
        obs = np.frombuffer(buf, rec, m, pos)
        pos += 24 * m
        images[iid] = Image(iid, qt[:4], qt[4:], cid, name, np.stack([obs["x"], obs["y"]], axis=1), obs["id"].astype(np.int64))
    return images


def read_points3d_bin(path):
    buf = open(path, "rb").read()
    (n,), pos = struct.unpack_from("<Q", buf, 0), 8
    points = {}
    for _ in range(n):
        pid, x, y, z, r, g, b, err, t = struct.unpack_from("<QdddBBBdQ", buf, pos)
        pos += 51
        track = np.frombuffer(buf, "<i4", 2 * t, pos).reshape(t, 2)
        pos += 8 * t
        points[pid] = Point3D(pid, np.array([x, y, z]), np.array([r, g, b]), err, track[:, 0].copy(), track[:, 1].copy())
    return points


def read_model(model_dir):
    """(cameras, images, points3D) of ``<model_dir>/{cameras,images,points3D}.bin``, each a dict by id."""
    return (read_cameras_bin(os.path.join(model_dir, "cameras.bin")), read_images_bin(os.path.join(model_dir, "images.bin")),
            read_points3d_bin(os.path.join(model_dir, "points3D.bin")))


def write_model(model_dir, cameras, images, points3d):
    """The inverse of `read_model` (tests and synthetic scenes use it)."""
    os.makedirs(model_dir, exist_ok=True)
    with open(os.path.join(model_dir, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for c in cameras.values():
            f.write(struct.pack("<iiQQ", c.id, MODEL_IDS[c.model], c.width, c.height))
            f.write(np.asarray(c.params, "<f8").tobytes())
    with open(os.path.join(model_dir, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for im in images.values():
            f.write(struct.pack("<i", im.id) + np.asarray(im.qvec, "<f8").tobytes() + np.asarray(im.tvec, "<f8").tobytes())
            f.write(struct.pack("<i", im.camera_id) + im.name.encode("utf-8") + b"\x00" + struct.pack("<Q", len(im.point3D_ids)))
            rec = np.zeros(len(im.point3D_ids), np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")]))
            rec["x"], rec["y"], rec["id"] = im.xys[:, 0], im.xys[:, 1], im.point3D_ids
            f.write(rec.tobytes())
    with open(os.path.join(model_dir, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(points3d)))
        for p in points3d.values():
            f.write(struct.pack("<QdddBBBdQ", p.id, *[float(v) for v in p.xyz], *[int(v) for v in p.rgb], float(p.error), len(p.image_ids)))
            f.write(np.stack([p.image_ids, p.point2D_idxs], axis=1).astype("<i4").tobytes())


# ------------------------------------------------------------------ cameras (colmap2mvsnet.py:321-377)
def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


def intrinsic_of(cam):
    single = CAMERA_MODELS[MODEL_IDS[cam.model]][2]
    fx, fy, cx, cy = (cam.params[0], cam.params[0], cam.params[1], cam.params[2]) if single else cam.params[:4]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])


def extrinsic_of(image):
    e = np.zeros((4, 4))
    e[:3, :3] = qvec2rotmat(image.qvec)
    e[:3, 3] = image.tvec
    e[3, 3] = 1
    return e


def depth_range(K, E, xyz, max_d, interval_scale):
    """(depth_min, depth_interval, depth_num, depth_max) of one image from the (n,3) positions of its valid observations."""
    zs = np.sort(np.matmul(E, np.concatenate([xyz, np.ones((len(xyz), 1))], axis=1).T)[2])
    depth_min, depth_max = zs[int(len(zs) * .01)], zs[int(len(zs) * .99)]
    if max_d == 0:                         # as many hypotheses as one-pixel steps at depth_min span in inverse depth
        R, t = E[0:3, 0:3], E[0:3, 3]
        p1, p2 = [K[0, 2], K[1, 2], 1], [K[0, 2] + 1, K[1, 2], 1]
        P1 = np.matmul(np.linalg.inv(R), np.matmul(np.linalg.inv(K), p1) * depth_min - t)
        P2 = np.matmul(np.linalg.inv(R), np.matmul(np.linalg.inv(K), p2) * depth_min - t)
        depth_num = (1 / depth_min - 1 / depth_max) / (1 / depth_min - 1 / (depth_min + np.linalg.norm(P2 - P1)))
    else:
        depth_num = max_d
    return depth_min, (depth_max - depth_min) / (depth_num - 1) / interval_scale, depth_num, depth_max


# ------------------------------------------------------------------ view selection (colmap2mvsnet.py:379-408)
def observation_lists(images, points3d):
    """(offsets (N+1) int64, obs int32, points (M,3) float64): the images' observation lists in CSR form with the point ids
    replaced by rows of ``points`` (-1 stays -1); images in id order 1 .. N."""
    ids = np.array(sorted(points3d), np.int64)
    points = np.stack([points3d[k].xyz for k in ids]).astype(np.float64) if len(ids) else np.zeros((0, 3))
    offsets, lists = [0], []
    for i in range(1, len(images) + 1):
        pid = np.asarray(images[i].point3D_ids, np.int64)
        row = np.searchsorted(ids, pid)
        valid = pid != -1
        known = valid & (row < len(ids))
        known[known] = ids[row[known]] == pid[known]
        if (valid & ~known).any():
            raise ColmapError(f"image {i} ({images[i].name}) observes the 3-D point {int(pid[valid & ~known][0])}, which points3D.bin does not hold")
        lists.append(np.where(valid, row, -1).astype(np.int32))
        offsets.append(offsets[-1] + len(pid))
    obs = np.concatenate(lists) if lists else np.zeros(0, np.int32)
    return np.array(offsets, np.int64), obs, points


def camera_centres(extrinsics):
    return np.stack([-np.matmul(E[:3, :3].transpose(), E[:3, 3:4])[:, 0] for E in extrinsics])


def pair_terms_host(i, j, offsets, obs, points, centres, theta0, sigma1, sigma2):
    """The terms of score[i][j] in the order of image i's list (float64): what ufr_view_pair_scores adds up."""
    li, lj = obs[offsets[i]:offsets[i + 1]], obs[offsets[j]:offsets[j + 1]]
    p = li[(li >= 0) & (li < len(points)) & np.isin(li, lj)]
    x = points[p]
    u, v = centres[i] - x, centres[j] - x
    dot = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    nu = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
    nv = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = (180 / np.pi) * np.arccos(np.clip(dot / nu / nv, -1.0, 1.0))
    d = theta - theta0
    return np.exp(-d * d / (2 * np.where(theta <= theta0, sigma1, sigma2) ** 2))


def pair_scores_host(offsets, obs, points, centres, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """ufr_view_pair_scores on the host: each pair's terms added in the reference's order, one running float64 sum."""
    N = len(offsets) - 1
    score = np.zeros((N, N))
    for i in range(N):
        for j in range(i + 1, N):
            terms = pair_terms_host(i, j, offsets, obs, points, centres, theta0, sigma1, sigma2)
            score[i, j] = score[j, i] = np.add.accumulate(terms)[-1] if len(terms) else 0.0
    return score


# ------------------------------------------------------------------ the conversion
def cam_text(E, K, rng):
    lines = ["extrinsic"] + ["".join(str(E[j, k]) + " " for k in range(4)) for j in range(4)]
    lines += ["", "intrinsic"] + ["".join(str(K[j, k]) + " " for k in range(3)) for j in range(3)]
    return "\n".join(lines) + "\n\n%f %f %f %f\n" % tuple(rng)


def pair_text(view_sel):
    out = "%d\n" % len(view_sel)
    for i, sel in enumerate(view_sel):
        out += "%d\n%d " % (i, len(sel)) + "".join("%d %f " % (k, s) for k, s in sel) + "\n"
    return out


def read_pair_text(text):
    """[[(image, score)]] of a pair file's text, one list per reference view"""
    lines = text.splitlines()
    rows = []
    for i in range(int(lines[0])):
        tokens = lines[2 + 2 * i].split()
        rows.append([(int(k), float(s)) for k, s in zip(tokens[1::2], tokens[2::2])])
    return rows


def camera_zooms(cameras, images, fit):
    """{camera id: zoom} for ``--undistort``: 1 for a pinhole camera and for ``fit`` "keep", else `undistort.fit_zoom`."""
    from . import undistort as U

    zooms = {}
    for cid in sorted({im.camera_id for im in images.values()}):
        cam = cameras[cid]
        if cam.model not in U.SUPPORTED_MODELS:
            raise ColmapError(f"--undistort: camera {cid} has the model {cam.model}, which is not supported "
                              f"(supported: {', '.join(U.SUPPORTED_MODELS)})")
        try:
            U.split_params(cam.model, cam.params)
            keep = fit == "keep" or cam.model in PINHOLE_MODELS
            zooms[cid] = 1.0 if keep else U.fit_zoom(cam.model, cam.params, intrinsic_of(cam), int(cam.height), int(cam.width))
        except ValueError as e:
            raise ColmapError(f"--undistort: camera {cid} ({cam.model}): {e}") from None
    return zooms


def convert(dense_folder, max_d=0, interval_scale=1, theta0=5, sigma1=1, sigma2=10, write=True, convert_format=False, device="cuda",
            undistort=False, undistort_fit="inside"):
    """The conversion in memory; with ``write`` also on disk.  Returns a dict: ``intrinsics`` (N,3,3), ``extrinsics`` (N,4,4),
    ``depth_ranges`` (N,4) = (min, interval, number, max), ``score`` (N,N), ``view_sel`` (per image the up to 10 (image,
    score) pairs, best first), ``names``, the file texts ``cam_texts`` / ``pair_text``, ``intrinsics_source`` (N,3,3, what
    `intrinsic_of` reads from the model), ``zoom`` (N) and ``distorted_models`` (the names of the models in use that have lens
    distortion); image k of the output is COLMAP's image k + 1.

    With ``undistort`` the pictures are resampled to pinhole cameras (the module text): ``intrinsics``, the camera files and the
    depth ranges then describe those cameras, K' = K with both focal lengths times ``zoom``.  With ``write=False`` the dict also
    holds the arrays that would have been written: ``images`` (per image (H,W,3) uint8), ``masks`` and ``valid`` (per image
    (H,W) uint8), each None for an image of a pinhole camera, whose files are copied."""
    cameras, images, points3d = read_model(os.path.join(dense_folder, "sparse", "0"))
    N = len(images)
    if N < 1 or sorted(images) != list(range(1, N + 1)):
        raise ColmapError(f"{dense_folder}: the image ids of sparse/0/images.bin are not 1 .. {N} (the converter indexes images[i + 1])")
    for im in images.values():
        if im.camera_id not in cameras:
            raise ColmapError(f"image {im.id} ({im.name}) names camera {im.camera_id}, which cameras.bin does not hold")
    if not (sigma1 > 0 and sigma2 > 0):
        raise ColmapError(f"--sigma1 {sigma1} --sigma2 {sigma2}: both must be positive")
    if undistort_fit not in UNDISTORT_FITS:
        raise ColmapError(f"--undistort_fit {undistort_fit}: must be one of {', '.join(UNDISTORT_FITS)}")
    K_source = [intrinsic_of(cameras[images[i + 1].camera_id]) for i in range(N)]
    K, zoom = K_source, np.ones(N)
    if undistort:
        from .undistort import zoomed

        zooms = camera_zooms(cameras, images, undistort_fit)
        zoom = np.array([zooms[images[i + 1].camera_id] for i in range(N)])
        K = [zoomed(K_source[i], zoom[i]) for i in range(N)]
    E = [extrinsic_of(images[i + 1]) for i in range(N)]
    offsets, obs, points = observation_lists(images, points3d)
    ranges = []
    for i in range(N):
        li = obs[offsets[i]:offsets[i + 1]]
        li = li[li >= 0]
        if len(li) == 0:
            raise ColmapError(f"image {i + 1} ({images[i + 1].name}) has no observation of a 3-D point: no depth range")
        ranges.append(depth_range(K[i], E[i], points[li], max_d, interval_scale))
    centres = camera_centres(E)
    if str(device).startswith("cpu"):
        score = pair_scores_host(offsets, obs, points, centres, theta0, sigma1, sigma2)
    else:
        from . import ops

        score = ops.view_pair_scores(offsets, obs, points, centres, theta0, sigma1, sigma2, device=device).cpu().numpy()
    view_sel = []
    for i in range(N):
        order = np.argsort(score[i])[::-1]
        view_sel.append([(int(k), score[i, k]) for k in order[:TOP_VIEWS]])
    out = {"intrinsics": np.stack(K), "extrinsics": np.stack(E), "depth_ranges": np.array(ranges, np.float64), "score": score,
           "view_sel": view_sel, "names": [images[i + 1].name for i in range(N)],
           "cam_texts": [cam_text(E[i], K[i], ranges[i]) for i in range(N)], "pair_text": pair_text(view_sel),
           "intrinsics_source": np.stack(K_source), "zoom": zoom,
           "distorted_models": sorted({cameras[im.camera_id].model for im in images.values()} - set(PINHOLE_MODELS))}
    if undistort and not write:
        out["images"], out["masks"], out["valid"] = [None] * N, [None] * N, [None] * N
        for idx, dst, masks, valid in undistorted_groups(dense_folder, cameras, images, zoom, device):
            for j, i in enumerate(idx):
                out["images"][i], out["masks"][i], out["valid"][i] = dst[j], masks[j], valid
    if write:
        resampled = {i for i in range(N) if undistort and cameras[images[i + 1].camera_id].model not in PINHOLE_MODELS}
        if resampled and {"%08d.jpg" % i for i in range(N)} & set(out["names"]):
            raise ColmapError("--undistort: a picture's name is one of the names the converter writes (%08d.jpg): it would overwrite "
                              "a source it still has to read")
        _write(dense_folder, out, convert_format, set(range(N)) - resampled)
        if resampled:
            _write_undistorted(dense_folder, undistorted_groups(dense_folder, cameras, images, zoom, device))
    return out


def undistorted_groups(dense_folder, cameras, images, zoom, device):
    """``--undistort``: yields (image indices, pictures (n,H,W,3) uint8, masks (n,H,W) uint8, valid (H,W) uint8) for groups of at
    most 8 images that share a camera with lens distortion -- its pictures and, where there are any, their masks through
    `undistort.undistort_images` (so through ufr_image_undistort_u8 on a GPU).  An image without a mask file gets 255; every
    mask is 0 where ``valid`` is.  Images of pinhole cameras are in no group."""
    from . import undistort as U
    from .host_forms import imread_gray, imread_rgb

    image_dir, mask_dir = os.path.join(dense_folder, "images"), os.path.join(dense_folder, "masks")
    by_camera = {}
    for i in range(len(images)):
        by_camera.setdefault(images[i + 1].camera_id, []).append(i)
    for cid, members in sorted(by_camera.items()):
        cam = cameras[cid]
        if cam.model in PINHOLE_MODELS:
            continue
        H, W = int(cam.height), int(cam.width)
        for first in range(0, len(members), U.GROUP):
            idx = members[first:first + U.GROUP]
            pictures, masks = [], []
            for i in idx:
                name = images[i + 1].name
                src = os.path.join(image_dir, name)
                if not os.path.exists(src):
                    raise ColmapError(f"image {i + 1}: {src} is missing")
                pictures.append(imread_rgb(src))
                mask = os.path.join(mask_dir, name + ".png")
                masks.append(imread_gray(mask) if os.path.exists(mask) else None)
                for what, a in ((src, pictures[-1]), (mask, masks[-1])):
                    if a is not None and a.shape[:2] != (H, W):
                        raise ColmapError(f"image {i + 1}: {what} is {a.shape[1]}x{a.shape[0]}, camera {cid} is {W}x{H}: its "
                                          "parameters do not describe this file")
            z = float(zoom[idx[0]])
            dst, valid, _, _ = U.undistort_images(np.stack(pictures), cam, z, device)
            if any(m is not None for m in masks):
                stack = np.stack([np.full((H, W), 255, np.uint8) if m is None else m for m in masks])[..., None]
                out_masks = U.undistort_images(stack, cam, z, device)[0][..., 0]
            else:
                out_masks = np.broadcast_to(valid, (len(idx), H, W)).copy()
            yield idx, dst, out_masks, valid


def _copy(src, dst, convert_format):
    if convert_format:
        from PIL import Image as PilImage

        with PilImage.open(src) as im:
            im.convert("L" if im.mode in ("1", "L", "I", "I;16", "F") else "RGB").save(dst, format="JPEG")
    elif os.path.abspath(src) != os.path.abspath(dst):
        shutil.copyfile(src, dst)


def _write_undistorted(dense_folder, groups):
    from PIL import Image as PilImage

    image_dir, mask_dir = os.path.join(dense_folder, "images"), os.path.join(dense_folder, "masks")
    os.makedirs(mask_dir, exist_ok=True)
    for idx, dst, masks, _ in groups:
        for j, i in enumerate(idx):
            PilImage.fromarray(dst[j], "RGB").save(os.path.join(image_dir, "%08d.jpg" % i), format="JPEG", **JPEG_OPTIONS)
            PilImage.fromarray(masks[j], "L").save(os.path.join(mask_dir, "%08d_mask.jpg" % i), format="JPEG", **JPEG_OPTIONS)


def _write(dense_folder, out, convert_format, copied=None):
    """the text files, and the pictures and masks of the images ``copied`` (indices; None = all) under their new names"""
    cam_dir, image_dir, mask_dir = (os.path.join(dense_folder, d) for d in ("cams", "images", "masks"))
    os.makedirs(cam_dir, exist_ok=True)
    for i, text in enumerate(out["cam_texts"]):
        with open(os.path.join(cam_dir, "%08d_cam.txt" % i), "w") as f:
            f.write(text)
    for path in (os.path.join(dense_folder, "pair.txt"), os.path.join(cam_dir, "pair.txt")):    # the reference's place; its loader's
        with open(path, "w") as f:
            f.write(out["pair_text"])
    for i, name in enumerate(out["names"]):
        if copied is not None and i not in copied:
            continue
        src = os.path.join(image_dir, name)
        if not os.path.exists(src):
            raise ColmapError(f"image {i + 1}: {src} is missing")
        _copy(src, os.path.join(image_dir, "%08d.jpg" % i), convert_format)
        mask = os.path.join(mask_dir, name + ".png")
        if os.path.exists(mask):
            _copy(mask, os.path.join(mask_dir, "%08d_mask.jpg" % i), convert_format)


def make_parser():
    parser = argparse.ArgumentParser(description="Convert colmap camera")
    parser.add_argument("--dense_folder", type=str, help="Project dir.")
    parser.add_argument("--max_d", type=int, default=0)
    parser.add_argument("--interval_scale", type=float, default=1)
    parser.add_argument("--theta0", type=float, default=5)
    parser.add_argument("--sigma1", type=float, default=1)
    parser.add_argument("--sigma2", type=float, default=10)
    parser.add_argument("--test", action="store_true", default=False, help="If set, do not write to file.")
    parser.add_argument("--convert_format", action="store_true", default=False, help="If set, convert image to jpg format.")
    return parser


def make_command_parser():
    """`make_parser()`, the reference's flags, and ours"""
    parser = make_parser()
    parser.add_argument("--undistort", action="store_true", default=False,
                        help="Resample the pictures of cameras with lens distortion to pinhole cameras (COLMAP's undistorter has not run).")
    parser.add_argument("--undistort_fit", type=str, default="inside",
                        help="inside: zoom in until no blank pixel is left on the border (default); keep: keep the focal length.")
    return parser


def main(argv=None):
    parser = make_command_parser()
    args = parser.parse_args(argv)
    if not args.dense_folder:
        parser.error("--dense_folder is required")
    try:
        out = convert(args.dense_folder, args.max_d, args.interval_scale, args.theta0, args.sigma1, args.sigma2, write=not args.test,
                      convert_format=args.convert_format, device="cuda:0", undistort=args.undistort, undistort_fit=args.undistort_fit)
    except ColmapError as e:
        parser.error(str(e))
    except FileNotFoundError as e:
        parser.error(f"{e.filename} is missing under --dense_folder {args.dense_folder}")
    N = len(out["names"])
    if not args.undistort and out["distorted_models"]:
        print("note: the camera model %s has lens distortion, and the camera files written describe pinhole cameras: run COLMAP's "
              "undistorter first, or pass --undistort" % ", ".join(out["distorted_models"]), file=sys.stderr)
    print("%d images, depth range of image 0: %f .. %f in %f steps; best views of image 0: %s%s" % (
        N, out["depth_ranges"][0][0], out["depth_ranges"][0][3], out["depth_ranges"][0][2],
        " ".join("%d" % k for k, _ in out["view_sel"][0]), "" if not args.test else " (--test: nothing written)"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
