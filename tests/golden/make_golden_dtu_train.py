"""Records the reference's own `MVSDataset` (code1/dataset/dtu_train.py) on a small synthetic DTU training tree into
dtu_train_small.npz, together with the tree's text files and the recipe of its pictures and depth maps.

    python tests/golden/make_golden_dtu_train.py /path/to/reference

Run where the reference tree is; the tests read only the .npz.  Nothing of the reference's text is written anywhere.

The tree (tests/dtu_train_golden.py rebuilds it): two scans; `Cameras/train/%08d_cam.txt` for all 49 views (the loader reads
them all), look-at cameras about 650 mm from the origin with DTU's quarter-size intrinsics; `Cameras/pair.txt` with ten
sources per view; `Rectified/<scan>_train/rect_%03d_<light>_r5000.png`, 640x512, and `Depths_raw/<scan>/depth_map_%04d.pfm`,
1600x1200, only for the views the recorded items read.  Pictures and depth maps are integer hash formulas of (scan, view,
light, x, y) -- `picture` and `depth_map` below -- so the tests regenerate them instead of storing 50 MB; the depth maps have
holes (0) and values on both sides of the cameras' depth range.

Two cases: split "test" with test_ref_views [23, 24, 33] (light 3; the source list is replaced by the reference views) and
split "train" with n_views 5 ('best' selection, 7 lights).  Of each, the items ITEMS[case] are recorded: every small tensor
whole; `images`, `depths_h`, `ray_d`, `cam_ray_d` (and ref_img / source_imgs, which are slices of images) at a fixed pixel
set -- the first / last row and column and 4096 seeded pixels -- for the items PIXEL_ITEMS[case] (shape and dtype for all):
the pictures as their 8-bit values (the generator checks that value / 255 in float32 is what the loader returned), the
other three, which the reference leaves in float64, rounded to float32.  `len` and every item's meta are recorded for both
cases.

How the reference is made to run: `cv2` is a stand-in of two functions (resize for INTER_NEAREST at fx = fy = 0.5: source
pixel (2y, 2x); decomposeProjectionMatrix: uforecon_amd.cameras' restatement), `torchvision` one of `T.Compose` /
`T.ToTensor` (/ 255 in float32) and empty names, `termcolor.colored` the identity.  The class then runs through
`DataLoader(batch_size=1, num_workers=0)`.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SCANS = ["scan3", "scan9"]
IMG_WH = (640, 512)
PFM_WH = (1600, 1200)
CASES = {
    "test": dict(split="test", n_views=3, test_ref_views=[23, 24, 33], view_selection_type="best"),
    "train": dict(split="train", n_views=5, test_ref_views=[], view_selection_type="best"),
}
ITEMS = {"test": [0, 4], "train": [7, 49 * 2 * 2 + 49 + 30]}      # (scan3, ref 23), (scan9, ref 24); (light 0, scan3, ref 7), (light 2, scan9, ref 30)
PIXEL_ITEMS = {"test": [4], "train": [275]}                      # the items whose per-pixel tensors are recorded (the others: shape and dtype)
N_SEEDED = 4096
PIXEL_KEYS = {"images": 2, "ref_img": 1, "source_imgs": 2, "depths_h": 1, "ray_d": 1, "cam_ray_d": 1}   # key -> leading dims before the pixels


def _hash(a):
    a = (a ^ (a >> np.uint64(15))) * np.uint64(0x2C1B3C6D)
    a = (a ^ (a >> np.uint64(12))) * np.uint64(0x297A2D39)
    return (a ^ (a >> np.uint64(15))) & np.uint64(0xFFFFFFFF)


def _grid(h, w, seed):
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    return (y * np.uint64(w) + x) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)


def picture(scan_idx, vid, light):
    """(512, 640, 3) uint8"""
    with np.errstate(over="ignore"):
        g = _grid(IMG_WH[1], IMG_WH[0], 1 + scan_idx * 1000 + vid * 10 + light)
        return np.stack([_hash(g + np.uint64(c * 7919)) & np.uint64(255) for c in range(3)], -1).astype(np.uint8)


def depth_map(scan_idx, vid):
    """(1200, 1600) float32, in the order of the picture (top row first): 250 .. 1250 mm in steps of 1/64, a seventh of the
    pixels 0"""
    with np.errstate(over="ignore"):
        g = _grid(PFM_WH[1], PFM_WH[0], 500 + scan_idx * 100 + vid)
        h = _hash(g)
        d = np.float32(250.0) + (h % np.uint64(1000 * 64)).astype(np.float32) / np.float32(64.0)
        d[_hash(g + np.uint64(12345)) % np.uint64(7) == 0] = 0.0
        return d.astype(np.float32)


def write_pfm(path, image):
    """little-endian grey PFM: the rows bottom-up, as read_pfm expects"""
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.0\n" % (image.shape[1], image.shape[0]))
        f.write(np.ascontiguousarray(np.flipud(image)).astype("<f4").tobytes())


def look_at(eye):
    z = -eye / np.linalg.norm(eye)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ eye
    return E


def camera_texts(rng):
    """{view id: text of %08d_cam.txt}: DTU's intrinsics at a quarter of 640x512 (the loader multiplies them by 4)"""
    K = np.array([[361.54125, 0, 82.900625], [0, 360.3975, 66.383875], [0, 0, 1]])
    cams = {}
    for vid in range(49):
        a, b = 0.09 * (vid % 7 - 3), 0.25 + 0.06 * (vid // 7)
        eye = 650.0 * np.array([np.sin(a) * np.cos(b), -np.cos(a) * np.cos(b), np.sin(b)]) + rng.uniform(-10, 10, 3)
        E = look_at(eye)
        lines = ["extrinsic"] + [" ".join(repr(float(v)) for v in row) for row in E] + ["", "intrinsic"]
        lines += [" ".join(repr(float(v)) for v in row) for row in K] + ["", "%s 2.5" % repr(425.0 + 0.25 * (vid % 5)), ""]
        cams[vid] = "\n".join(lines)
    return cams


def pair_text(rng):
    lines = ["49"]
    for ref in range(49):
        src = [int(v) for v in rng.permutation([i for i in range(49) if i != ref])[:10]]
        lines += [str(ref), "10 " + " ".join("%d %s" % (s, repr(round(2000.0 - 37.5 * k, 2))) for k, s in enumerate(src))]
    return "\n".join(lines) + "\n"


def write_tree(root, cams, pairs, needed):
    """``needed``: [(scan index, view, light)] -- the pictures (and those views' depth maps) to write"""
    from PIL import Image

    os.makedirs(os.path.join(root, "Cameras", "train"), exist_ok=True)
    for vid, text in cams.items():
        with open(os.path.join(root, "Cameras", "train", "%08d_cam.txt" % int(vid)), "w") as f:
            f.write(text)
    with open(os.path.join(root, "Cameras", "pair.txt"), "w") as f:
        f.write(pairs)
    with open(os.path.join(root, "scans.txt"), "w") as f:
        f.write("\n".join(SCANS) + "\n")
    for si, vid, light in needed:
        scan = SCANS[si]
        os.makedirs(os.path.join(root, "Rectified", scan + "_train"), exist_ok=True)
        os.makedirs(os.path.join(root, "Depths_raw", scan), exist_ok=True)
        Image.fromarray(picture(si, vid, light)).save(os.path.join(root, "Rectified", scan + "_train", "rect_%03d_%d_r5000.png" % (vid + 1, light)))
        pfm = os.path.join(root, "Depths_raw", scan, "depth_map_%04d.pfm" % vid)
        if not os.path.exists(pfm):
            write_pfm(pfm, depth_map(si, vid))


def pixel_set():
    """flat indices into 512 x 640: the first / last row and column, then N_SEEDED hashed ones"""
    W, H = IMG_WH
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    border = np.flatnonzero(((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).reshape(-1))
    with np.errstate(over="ignore"):
        seeded = _hash(np.arange(N_SEEDED, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(99)) % np.uint64(H * W)
    return np.concatenate([border, seeded.astype(np.int64)])


def import_reference_loader(ref_root):
    import torch

    from uforecon_amd import cameras

    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST = 0

    def resize(image, dsize, fx, fy, interpolation):
        assert dsize is None and fx == 0.5 and fy == 0.5 and interpolation == cv2.INTER_NEAREST
        return np.ascontiguousarray(image[0::2, 0::2][:int(np.rint(image.shape[0] * 0.5)), :int(np.rint(image.shape[1] * 0.5))])

    cv2.resize = resize
    cv2.decomposeProjectionMatrix = lambda P: cameras.decompose_projection_matrix(P)
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.InterpolationMode = None

    def compose(fs):
        def run(im):
            for f in fs:
                im = f(im)
            return im
        return run

    tv.transforms.Compose = compose
    tv.transforms.ToTensor = lambda: (lambda im: torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255))
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    tv.transforms.functional.resize = tv.transforms.functional.pil_to_tensor = None
    for m in (tv, tv.transforms, tv.transforms.functional):
        sys.modules[m.__name__] = m
    tc = types.ModuleType("termcolor")
    tc.colored = lambda text, *a, **k: text
    sys.modules["termcolor"] = tc
    sys.path.insert(0, ref_root)
    from code1.dataset import dtu_train as mod

    return mod.MVSDataset


def views_of(meta, case):
    scan, light, ref, src = meta
    views = [ref] + (src[:case["n_views"] - 1] if case["split"] == "train" else src)
    return [(SCANS.index(scan), v, light) for v in views]


def main():
    import torch
    from torch.utils.data import DataLoader, Subset

    ref_root = sys.argv[1]
    MVSDataset = import_reference_loader(ref_root)
    rng = np.random.default_rng(31)
    cams, pairs = camera_texts(rng), pair_text(rng)
    pix = pixel_set()
    out = {"scans": np.array(json.dumps(SCANS)), "cases": np.array(json.dumps(CASES)), "items": np.array(json.dumps(ITEMS)),
           "pair_txt": np.array(pairs), "pixels": pix}
    for vid in range(49):
        out["cam/%d" % vid] = np.array(cams[vid])
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, cams, pairs, [])
        needed = []
        for name, case in CASES.items():
            ds = MVSDataset(root_dir=root, split_filepath=os.path.join(root, "scans.txt"), pair_filepath=os.path.join(root, "Cameras", "pair.txt"),
                            **{k: (list(v) if isinstance(v, list) else v) for k, v in case.items()})
            out[f"{name}/len"] = np.array(len(ds))
            out[f"{name}/metas"] = np.array(json.dumps([[m[0], int(m[1]), int(m[2]), [int(s) for s in m[3]]] for m in ds.metas]))
            here = sorted({t for i in ITEMS[name] for t in views_of(ds.metas[i], case)})
            write_tree(root, cams, pairs, here)
            needed += here
            for i, batch in zip(ITEMS[name], DataLoader(Subset(ds, ITEMS[name]), batch_size=1, num_workers=0)):
                for k, v in batch.items():
                    pre = f"{name}/{i}/{k}"
                    if k == "proj_matrices":
                        for st, t in v.items():
                            out[f"{pre}.{st}"] = t.numpy()
                    elif k == "meta":
                        assert isinstance(v, list) and len(v) == 1
                        out[pre] = np.array(v[0])
                    elif k in PIXEL_KEYS:
                        a = v.numpy()
                        lead = 1 + PIXEL_KEYS[k]                                   # the collated batch axis in front
                        out[pre + ".shape"], out[pre + ".dtype"] = np.array(a.shape), np.array(str(a.dtype))
                        if k in ("ref_img", "source_imgs"):                        # slices of images
                            assert np.array_equal(a, batch["images"].numpy()[:, 0] if k == "ref_img" else batch["images"].numpy()[:, 1:])
                            continue
                        if i not in PIXEL_ITEMS[name]:
                            continue
                        a = a.reshape(a.shape[:lead] + (-1,))[..., pix]
                        if k == "images":
                            k8 = np.rint(a.astype(np.float64) * 255).astype(np.uint8)
                            assert np.array_equal(k8.astype(np.float32) / np.float32(255), a)
                            a = k8
                        else:                                                      # float64 in the reference: its float32 rounding
                            assert a.dtype == np.float64
                            a = a.astype(np.float32)
                        out[pre] = a
                    else:
                        assert isinstance(v, torch.Tensor), (k, type(v))
                        out[pre] = v.numpy()
                        print(name, i, k, v.dtype, tuple(v.shape))
        out["needed"] = np.array(sorted(set(needed)))
    for k in sorted(out):
        if "/" in k and k.split("/")[-1].split(".")[0] in PIXEL_KEYS:
            print(k, out[k].dtype, out[k].shape)
    path = os.path.join(HERE, "dtu_train_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
