"""What tests/test_dtu_train.py and tests/test_gpu_dtu_train.py share: tests/golden/dtu_train_small.npz (written by
tests/golden/make_golden_dtu_train.py) read once, and the synthetic training tree rebuilt from it -- the text files from the
fixture, the pictures and depth maps from the generator's own integer formulas."""
import functools
import importlib.util
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PIXEL_KEYS = ("images", "depths_h", "ray_d", "cam_ray_d")


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_golden_dtu_train", os.path.join(HERE, "golden", "make_golden_dtu_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(HERE, "golden", "dtu_train_small.npz"))
    return {k: z[k] for k in z.files}


def cases():
    return json.loads(str(golden()["cases"]))


def items():
    return json.loads(str(golden()["items"]))


def metas(case):
    return [(m[0], m[1], m[2], m[3]) for m in json.loads(str(golden()[f"{case}/metas"]))]


def write_tree(tmp_path):
    """the tree as the generator wrote it (every picture and depth map the recorded items read); returns its root"""
    g = golden()
    root = os.path.join(str(tmp_path), "dtu_training")
    cams = {int(k[4:]): str(v) for k, v in g.items() if k.startswith("cam/")}
    generator().write_tree(root, cams, str(g["pair_txt"]), [tuple(int(v) for v in t) for t in g["needed"]])
    return root


def open_dataset(root, case, device, **over):
    from uforecon_amd.dtu_train import DtuTrain

    kw = dict(cases()[case], split_filepath=os.path.join(root, "scans.txt"), pair_filepath=os.path.join(root, "Cameras", "pair.txt"))
    kw.update(over)
    return DtuTrain(root, device=device, **kw)


def golden_item(case, i):
    pre = f"{case}/{i}/"
    return {k[len(pre):]: (str(v) if k.endswith("/meta") else v) for k, v in golden().items() if k.startswith(pre)}


def flat_batch(batch):
    out = {}
    for k, v in batch.items():
        if k == "proj_matrices":
            out.update({f"proj_matrices.{st}": t.cpu().numpy() for st, t in v.items()})
        elif k == "meta":
            assert isinstance(v, list) and len(v) == 1
            out[k] = v[0]
        else:
            out[k] = v.cpu().numpy()
    return out


def at_pixels(a, lead):
    """the recorded pixel set of an array whose last dims are the pixels: (..., H, W) or (..., H*W) -> (..., n)"""
    return a.reshape(a.shape[:lead] + (-1,))[..., golden()["pixels"]]
