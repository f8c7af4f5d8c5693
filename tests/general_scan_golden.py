"""What tests/test_general_scan.py, tests/test_colmap2mvsnet.py and their GPU counterparts share: the two golden files
(tests/golden/general_scan_small.npz, tests/golden/colmap_small.npz; written by tests/golden/make_golden_general_scan.py and
make_golden_colmap.py) read once, and the scene directories rebuilt from them."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def golden(name="general_scan_small"):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    return {k: z[k] for k in z.files}


def cases():
    return json.loads(str(golden()["cases"]))


def write_files(directory, g):
    """every `file/<relative path>` entry of a golden dict under ``directory``: a str array is the file's text (or, as
    "@<relative path>", the bytes of that other file), a uint8 array its bytes"""
    for k, v in g.items():
        if not k.startswith("file/"):
            continue
        path = os.path.join(directory, k[5:])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if v.dtype.kind == "U" and str(v).startswith("@"):
            v = g["file/" + str(v)[1:]]
        if v.dtype.kind == "U":
            with open(path, "w") as f:
                f.write(str(v))
        else:
            with open(path, "wb") as f:
                f.write(v.tobytes())


def write_scene(tmp_path):
    """<tmp>/<root name>/<scan>/{cams,images,masks,blended_images}, as the generator wrote them; returns (root, scan)."""
    g = golden()
    root, scan = os.path.join(str(tmp_path), str(g["root_name"])), str(g["scan"])
    write_files(os.path.join(root, scan), g)
    return root, scan


def open_scan(root, scan, case, device):
    from uforecon_amd.general_scan import GeneralScan

    return GeneralScan(root, scan, device=device, **cases()[case])


def metas(case):
    return [(r, s) for r, s in json.loads(str(golden()[case + "/metas"]))]


def golden_batch(case, i):
    """{key: array} of batch ``i``; proj_matrices as `proj_matrices.stageN`, meta as a str"""
    pre = f"{case}/{i}/"
    return {k[len(pre):]: (str(v) if k.endswith("/meta") else v) for k, v in golden().items() if k.startswith(pre)}


def write_colmap_scene(tmp_path):
    """<tmp>/colmap_small/{sparse/0/*.bin, images/<name>, masks/<name>.png} of colmap_small.npz; returns the dense folder."""
    dense = os.path.join(str(tmp_path), "colmap_small")
    write_files(dense, golden("colmap_small"))
    return dense
