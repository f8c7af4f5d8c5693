"""Records the reference's own `GeneralFit` (code1/dataset/general_fit.py) on a small synthetic scene into
general_scan_small.npz, together with the scene itself.

    python tests/golden/make_golden_general_scan.py /path/to/reference

Run where the reference tree is; the tests read only the .npz.  Nothing of the reference's text is written anywhere.

The scene: five look-at cameras about 650 mm from the origin (DTU-like units, so that the TSDF fusion's default voxel size
works) as ``cams/%08d_cam.txt`` with DTU's intrinsics scaled to 128x60 pictures and four-token depth lines ``near interval
number far`` that differ from file to file (the loader takes `depth_min` / `depth_interval` from the last file it read and
near / far from each file's first and last token), a ``cams/pair.txt`` with four sources per view, and random 8-bit pictures
(4x4 blocks plus a little noise) stored as 4:4:4 JPEG bytes under both layouts (``blended_images/%08d_masked.jpg``; ``images/%08d.jpg`` with single-channel
``masks/%08d_mask.jpg``).  Two cases:

  mvimage     dataset mvimage, use_mask, n_views 3, test_ref_view [0, 2, 3], 128x60 -> 64x32 (factors 2 and 1.875: the general
              resize path).  Three batches; the sources of each are test_ref_view, so view_ids = [0, 0, 2], [2, 0, 2], [3, 0, 2]:
              the reference view repeats
  blendedmvs  dataset blendedmvs, no mask, n_views 2, test_ref_view [] (every entry of the pair file with its own sources),
              128x60 -> 64x30 (both factors exactly 2: the box mean).  Five batches

How the reference is made to run: `cv2` is a stand-in module of four functions, each a call into the project's host
restatements (imread colour / grey, resize, decomposeProjectionMatrix); `einops.repeat` is the real one when einops is
installed, else a two-line stand-in.  GeneralFit fixes its picture size by dataset (768x576 / 960x544), so after constructing
the class this script OVERWRITES the instance's size attributes (img_wh, img_W, img_H) and its pixel table (w_mesh_flat,
h_mesh_flat, homo_pixel) for the small target, with the constructor's own expressions evaluated at that size.  The class then
runs through `DataLoader(batch_size=1, num_workers=0)`, and every tensor of every batch is recorded.

What this pins and what it does not.  PINNED to the reference, because they went through its own code: all the camera
arithmetic (inverses, the bounding box from the files' near / far, the scaled cameras, the poses), the schema (keys, shapes,
dtypes, meta), the ray tables, the filter and the source replacement of build_list, and the quirks
uforecon_amd/general_scan.py lists.  NOT pinned: the image values (they come from the restated resize and the restated grey
level, times the reference's own / 255 and / 254, so only the restatements are pinned) and the projection-matrix decomposition
(pinned only to the restatement's float32 rounding).
"""
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ROOT_NAME = "general_small"   # basename of the test directory: it is part of `meta`
SCAN = "scene7"
ORIGINAL_WH = (128, 60)
N_IMAGES = 5
CASES = {
    "mvimage": dict(n_views=3, test_ref_view=[0, 2, 3], dataset="mvimage", use_mask=True, img_wh=[64, 32]),
    "blendedmvs": dict(n_views=2, test_ref_view=[], dataset="blendedmvs", use_mask=False, img_wh=[64, 30]),
}


def look_at(eye):
    z = -eye / np.linalg.norm(eye)                      # the camera looks at the origin
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                             # world -> camera
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ eye
    return E


def jpeg_bytes(array):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(array).save(buf, format="JPEG", quality=95, subsampling=0)
    return np.frombuffer(buf.getvalue(), np.uint8)


def synthetic_scene(rng):
    """{relative path: file text (str) or file bytes (uint8 array)} of <root>/<scan>"""
    K = np.array([[2892.33 * ORIGINAL_WH[0] / 1600, 0, 823.205 * ORIGINAL_WH[0] / 1600],
                  [0, 2883.175 * ORIGINAL_WH[1] / 1200, 619.071 * ORIGINAL_WH[1] / 1200], [0, 0, 1]])
    files = {}
    for k in range(N_IMAGES):
        a = 0.35 * (k - 2)
        eye = 650.0 * np.array([np.sin(a), -np.cos(a) * np.cos(0.2 + 0.05 * k), np.sin(0.2 + 0.05 * k)]) + rng.uniform(-15, 15, 3)
        E = look_at(eye)
        near, interval, number = 420.0 + 3 * k, 2.4 + 0.05 * k, 192.0
        lines = ["extrinsic"] + [" ".join(str(float(v)) for v in row) + " " for row in E] + ["", "intrinsic"]
        lines += [" ".join(str(float(v)) for v in row) + " " for row in K]
        files["cams/%08d_cam.txt" % k] = "\n".join(lines) + "\n\n%f %f %f %f\n" % (near, interval, number, near + interval * (number - 1))
        blocks = np.kron(rng.integers(8, 248, (ORIGINAL_WH[1] // 4, ORIGINAL_WH[0] // 4, 3)), np.ones((4, 4, 1), np.int64))
        picture = (blocks + rng.integers(-8, 9, blocks.shape)).astype(np.uint8)      # 4x4 blocks plus a little noise: small files
        files["images/%08d.jpg" % k] = jpeg_bytes(picture)
        files["blended_images/%08d_masked.jpg" % k] = "@images/%08d.jpg" % k        # the same bytes under the other layout's name
        mask = rng.choice(np.array([0, 128, 254, 255], np.uint8), (ORIGINAL_WH[1] // 4, ORIGINAL_WH[0] // 4))
        files["masks/%08d_mask.jpg" % k] = jpeg_bytes(np.kron(mask, np.ones((4, 4), np.uint8)))
    pair = "%d\n" % N_IMAGES
    for k in range(N_IMAGES):
        others = sorted((j for j in range(N_IMAGES) if j != k), key=lambda j: (abs(j - k), j))
        pair += "%d\n%d " % (k, len(others)) + "".join("%d %f " % (j, 100.0 / abs(j - k)) for j in others) + "\n"
    files["cams/pair.txt"] = pair
    return files


def write_scene(root, files):
    for rel, content in files.items():
        path = os.path.join(root, SCAN, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if isinstance(content, str) and content.startswith("@"):      # "@<relative path>": the bytes of that file
            content = files[content[1:]]
        if isinstance(content, str):
            with open(path, "w") as f:
                f.write(content)
        else:
            with open(path, "wb") as f:
                f.write(np.asarray(content, np.uint8).tobytes())


def import_reference_loader(ref_root):
    from uforecon_amd import cameras, host_forms as D

    def resize(image, size):
        return D.resize_u8(image, size) if image.ndim == 3 else D.resize_u8(image[..., None], size)[..., 0]

    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda path, flag=1: D.imread_gray(path) if flag == 0 else np.ascontiguousarray(D.imread_rgb(path)[:, :, ::-1])
    cv2.resize = resize
    cv2.decomposeProjectionMatrix = lambda P: cameras.decompose_projection_matrix(P)
    sys.modules["cv2"] = cv2
    try:
        import einops  # noqa: F401
    except ImportError:
        einops = types.ModuleType("einops")
        einops.repeat = lambda t, pattern, L: t[None].expand(L, *t.shape)     # only "X Y -> L X Y" is asked
        sys.modules["einops"] = einops
    sys.path.insert(0, ref_root)
    from code1.dataset.general_fit import GeneralFit

    return GeneralFit


def shrink(ds, img_wh):
    """the constructor's size attributes and pixel table (general_fit.py:75-81), evaluated for ``img_wh``"""
    ds.img_wh = list(img_wh)
    ds.img_W, ds.img_H = ds.img_wh
    h_line = (np.linspace(0, ds.img_H - 1, ds.img_H)) * 2 / (ds.img_H - 1) - 1
    w_line = (np.linspace(0, ds.img_W - 1, ds.img_W)) * 2 / (ds.img_W - 1) - 1
    h_mesh, w_mesh = np.meshgrid(h_line, w_line, indexing="ij")
    ds.w_mesh_flat, ds.h_mesh_flat = w_mesh.reshape(-1), h_mesh.reshape(-1)
    ds.homo_pixel = np.stack([ds.w_mesh_flat, ds.h_mesh_flat, np.ones(len(ds.h_mesh_flat)), np.ones(len(ds.h_mesh_flat))])


def main():
    import torch
    from torch.utils.data import DataLoader

    ref_root = sys.argv[1]
    GeneralFit = import_reference_loader(ref_root)
    files = synthetic_scene(np.random.default_rng(31))
    out = {"root_name": np.array(ROOT_NAME), "scan": np.array(SCAN), "cases": np.array(json.dumps(CASES))}
    for rel, content in files.items():
        out["file/" + rel] = np.array(content) if isinstance(content, str) else content
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, ROOT_NAME)
        write_scene(root, files)
        for name, case in CASES.items():
            ds = GeneralFit(root_dir=root, scan_id=SCAN, n_views=case["n_views"], test_ref_view=list(case["test_ref_view"]),
                            dataset=case["dataset"], use_mask=case["use_mask"])
            shrink(ds, case["img_wh"])
            out[f"{name}/metas"] = np.array(json.dumps(ds.metas))
            for i, batch in enumerate(DataLoader(ds, batch_size=1, num_workers=0)):
                for k, v in batch.items():
                    if k == "proj_matrices":
                        for st, t in v.items():
                            out[f"{name}/{i}/proj_matrices.{st}"] = t.numpy()
                    elif k == "meta":
                        assert isinstance(v, list) and len(v) == 1
                        out[f"{name}/{i}/meta"] = np.array(v[0])
                    else:
                        assert isinstance(v, torch.Tensor), (k, type(v))
                        out[f"{name}/{i}/{k}"] = v.numpy()
            assert i + 1 == len(ds.metas)
    path = os.path.join(HERE, "general_scan_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
