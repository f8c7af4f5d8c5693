"""Records the reference's own `DtuFitSparse` (code1/dataset/dtu_test_sparse.py) on a small synthetic scan into
dtu_scan_small.npz, together with the scan itself and the flags of main.py's parser.

    python tests/golden/make_golden_dtu_scan.py /path/to/reference

Run where the reference tree is; the tests read only the .npz.  Nothing of the reference's text is written anywhere.

The scan: five look-at cameras about 650 mm from the origin (ids 23, 24, 33 for set 0 and 43, 42 for set 1) as `%08d_cam.txt`
with DTU's intrinsics scaled to 128x60 pictures, depth line `425.0 2.5` (`430.0 2.4` in camera 33, the last one set 0 reads:
the loader takes its depth range from the last file), and random 8-bit pictures.  Two cases:

  set0  n_views 3, views [23, 24, 33], 128x60 -> img_wh 64x32: DTU's own factors 2 and 1.875 (the general resize path)
  set1  n_views 2, set=1, 128x60 -> img_wh 64x30 (both factors exactly 2: the box mean), clip_wh (4, 2)

How the reference is made to run: `cv2` is a stand-in module of exactly three functions, each a call into
uforecon_amd's host restatements (imread, resize, decomposeProjectionMatrix); `torchvision.transforms` holds empty
names; and the module's `torch.from_numpy` passes tensors through, because dtu_test_sparse.py:389 hands it something that
load_scene (:294) has already made a tensor -- as shipped, the class raises TypeError on every torch.  The class then runs
through `DataLoader(batch_size=1, num_workers=0)`, and every tensor of every render view's batch is recorded.

What this pins and what it does not.  PINNED to the reference, because they went through its own code: all the camera
mathematics (inverses, the bounding box, the scaled cameras, the poses), the schema (keys, shapes, dtypes, meta), the ray
tables and the quirks uforecon_amd/dtu_scan.py lists.  NOT pinned: the image values (they come from the restated resize, so
only the restatement is pinned) and the decomposition (pinned only to the restatement's float32 rounding).
"""
import ast
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ROOT_NAME = "dtu_small"       # basename of the scan directory: it is part of `meta`
SCAN = "scan7"
ORIGINAL_WH = (128, 60)
VIEW_IDS = [23, 24, 33, 43, 42]
CASES = {
    "set0": dict(n_views=3, img_wh=[64, 32], clip_wh=[0, 0], set=0, test_view_pair=[23, 24, 33]),
    "set1": dict(n_views=2, img_wh=[64, 30], clip_wh=[4, 2], set=1, test_view_pair=None),
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


def synthetic_scan(rng):
    """({view id: camera file text}, {view id: (60,128,3) uint8})"""
    K = np.array([[2892.33 * ORIGINAL_WH[0] / 1600, 0, 823.205 * ORIGINAL_WH[0] / 1600],
                  [0, 2883.175 * ORIGINAL_WH[1] / 1200, 619.071 * ORIGINAL_WH[1] / 1200], [0, 0, 1]])
    cams, imgs = {}, {}
    for k, vid in enumerate(VIEW_IDS):
        a = 0.35 * (k - 2)
        eye = 650.0 * np.array([np.sin(a), -np.cos(a) * np.cos(0.2 + 0.05 * k), np.sin(0.2 + 0.05 * k)]) + rng.uniform(-15, 15, 3)
        E = look_at(eye)
        lines = ["extrinsic"] + [" ".join(repr(float(v)) for v in row) for row in E] + ["", "intrinsic"]
        lines += [" ".join(repr(float(v)) for v in row) for row in K] + ["", "430.0 2.4" if vid == 33 else "425.0 2.5", ""]
        cams[vid] = "\n".join(lines)
        imgs[vid] = rng.integers(0, 256, (ORIGINAL_WH[1], ORIGINAL_WH[0], 3), dtype=np.uint8)
    return cams, imgs


def write_scan(root, cams, imgs):
    """The directory layout `DtuFitSparse` reads: <root>/cameras/%08d_cam.txt, <root>/<scan>/image/%06d.png."""
    from PIL import Image

    os.makedirs(os.path.join(root, "cameras"), exist_ok=True)
    os.makedirs(os.path.join(root, SCAN, "image"), exist_ok=True)
    for vid, text in cams.items():
        with open(os.path.join(root, "cameras", "%08d_cam.txt" % vid), "w") as f:
            f.write(text)
        Image.fromarray(imgs[vid]).save(os.path.join(root, SCAN, "image", "%06d.png" % vid))


def import_reference_loader(ref_root):
    import torch

    from uforecon_amd import cameras, host_forms as D

    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda path: np.ascontiguousarray(D.imread_rgb(path)[:, :, ::-1])
    cv2.resize = lambda image, size: D.resize_u8(image, size)
    cv2.decomposeProjectionMatrix = lambda P: cameras.decompose_projection_matrix(P)
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.InterpolationMode = None
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    tv.transforms.functional.resize = tv.transforms.functional.pil_to_tensor = None
    for m in (tv, tv.transforms, tv.transforms.functional):
        sys.modules[m.__name__] = m
    sys.path.insert(0, ref_root)
    from code1.dataset import dtu_test_sparse as mod

    class TolerantTorch:                                 # dtu_test_sparse.py:389
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def from_numpy(a):
            return a if isinstance(a, torch.Tensor) else torch.from_numpy(a)

    mod.torch = TolerantTorch()
    return mod.DtuFitSparse


def parser_flags(ref_root):
    """[{"flag", "default", "action", "type", "nargs", "choices"}] of every add_argument call in main.py, read from its text."""
    tree = ast.parse(open(os.path.join(ref_root, "main.py")).read())
    flags = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", None) == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            lit = lambda k: ast.literal_eval(kw[k]) if k in kw else None  # noqa: E731
            flags.append({"flag": ast.literal_eval(node.args[0]), "default": lit("default"), "action": lit("action"),
                          "type": getattr(kw.get("type"), "id", None), "nargs": lit("nargs"), "choices": lit("choices")})
    return sorted(flags, key=lambda f: f["flag"])


def main():
    import torch
    from torch.utils.data import DataLoader

    ref_root = sys.argv[1]
    DtuFitSparse = import_reference_loader(ref_root)
    cams, imgs = synthetic_scan(np.random.default_rng(20))
    out = {"root_name": np.array(ROOT_NAME), "scan": np.array(SCAN), "original_img_wh": np.array(ORIGINAL_WH),
           "cases": np.array(json.dumps(CASES)), "main_py_flags": np.array(json.dumps(parser_flags(ref_root)))}
    for vid in VIEW_IDS:
        out["cam/%d" % vid] = np.array(cams[vid])
        out["img/%d" % vid] = imgs[vid]
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, ROOT_NAME)
        write_scan(root, cams, imgs)
        for name, case in CASES.items():
            ds = DtuFitSparse(root_dir=root, split="test", scan_id=SCAN, original_img_wh=list(ORIGINAL_WH),
                              **{k: (list(v) if isinstance(v, list) else v) for k, v in case.items()})
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
            assert i + 1 == case["n_views"]
    path = os.path.join(HERE, "dtu_scan_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
