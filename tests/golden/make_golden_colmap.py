"""Records the reference's own colmap2mvsnet.py on a small synthetic COLMAP model into colmap_small.npz, together with the
model itself.

    python tests/golden/make_golden_colmap.py /path/to/reference

Run where the reference tree is; the tests read only the .npz.  Nothing of the reference's text is written anywhere.

The scene: six look-at cameras about 650 mm from the origin (DTU-like units), 7 degrees apart, two COLMAP cameras (id 1 PINHOLE,
id 2 SIMPLE_RADIAL: both intrinsic branches); 300 points in a ball of radius 120 around the origin; every image observes a
random 70 % of them in random order, with some -1 entries in between, and image 3 observes one point twice.  Six images, so
the top 10 of every row is the whole row.  The pictures are 128x60 JPEGs, three of them with a mask ``masks/<name>.png``.
The model is written with the project's own `colmap2mvsnet.write_model` and read by the REFERENCE's reader, which pins both
directions of the file layout.

How the reference is made to run: the script has no functions to import, so it runs through `runpy.run_path(...,
run_name="__main__")` with `sys.argv` set, twice (``--max_d 0`` and ``--max_d 64 --interval_scale 2``); `cv2` is an empty
stand-in module (the script calls it only under --convert_format, which is not run).  Recorded: every file the script wrote
-- the camera texts, pair.txt -- and the names of the pictures and masks it copied.

What this pins and what it does not.  PINNED to the reference: the reader (as far as the converter uses it), the intrinsics by
model, the extrinsics, the depth ranges and depth_num to the 6 decimals of ``%f``, the text formats, the ranking, and the
scores to ``%f`` (5e-7 absolute).  The smallest gap between two scores of one row is checked here to be far above that
(> 1e-3), so the ranking cannot hinge on the last digit.  NOT pinned: scores beyond 6 decimals, --convert_format's bytes.
The `acos` clamp of this project never acts on this scene (no argument is within 1e-9 of +-1).
"""
import io
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

WH = (128, 60)
N_IMAGES, N_POINTS = 6, 300
RUNS = {"default": [], "max_d": ["--max_d", "64", "--interval_scale", "2"]}


def look_at(eye):
    z = -eye / np.linalg.norm(eye)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z]), eye                      # world -> camera rotation, centre


def rotmat2qvec(R):
    """(w, x, y, z) of a rotation matrix with w >= 0: the usual branch on the trace and the largest diagonal term"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q if q[0] >= 0 else -q


def synthetic_model(rng):
    from uforecon_amd import colmap2mvsnet as C

    fx, fy, cx, cy = 2892.33 * WH[0] / 1600, 2883.175 * WH[1] / 1200, 823.205 * WH[0] / 1600, 619.071 * WH[1] / 1200
    cameras = {1: C.Camera(1, "PINHOLE", WH[0], WH[1], np.array([fx, fy, cx, cy])),
               2: C.Camera(2, "SIMPLE_RADIAL", WH[0], WH[1], np.array([0.5 * (fx + fy), cx, cy, 0.01]))}
    xyz = rng.normal(size=(N_POINTS, 3))
    xyz = 120.0 * xyz / np.linalg.norm(xyz, axis=1, keepdims=True) * rng.uniform(0, 1, (N_POINTS, 1)) ** (1 / 3)
    point_ids = np.sort(rng.choice(np.arange(1, 5 * N_POINTS), N_POINTS, replace=False))     # COLMAP's ids have gaps
    images, tracks = {}, {int(p): [] for p in point_ids}
    for k in range(N_IMAGES):
        a = 0.122 * (k - 2.5)
        eye = 650.0 * np.array([np.sin(a), -np.cos(a) * np.cos(0.2 + 0.03 * k), np.sin(0.2 + 0.03 * k)]) + rng.uniform(-15, 15, 3)
        R, c = look_at(eye)
        t = -R @ c
        seen = rng.permutation(N_POINTS)[:int(0.7 * N_POINTS)]
        ids = point_ids[seen].astype(np.int64)
        if k == 3:
            ids = np.concatenate([ids, ids[:1]])                       # one point observed twice
        ids = np.insert(ids, rng.integers(0, len(ids), 25), -1)        # observations without a 3-D point
        cam = (xyz[np.searchsorted(point_ids, np.where(ids < 0, point_ids[0], ids))] @ R.T + t)
        xys = np.stack([fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy], axis=1)
        images[k + 1] = C.Image(k + 1, rotmat2qvec(R), t, 1 + k % 2, "view_%c.jpg" % (97 + k), xys, ids)
        for o, p in enumerate(ids):
            if p >= 0:
                tracks[int(p)].append((k + 1, o))
    points3d = {}
    for n, p in enumerate(point_ids):
        tr = np.array(tracks[int(p)], np.int32).reshape(-1, 2)
        points3d[int(p)] = C.Point3D(int(p), xyz[n], rng.integers(0, 256, 3), float(rng.uniform(0.2, 1.5)), tr[:, 0], tr[:, 1])
    return cameras, images, points3d


def file_bytes(array, fmt, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(array).save(buf, format=fmt, **kw)
    return np.frombuffer(buf.getvalue(), np.uint8)


def main():
    from uforecon_amd import colmap2mvsnet as C

    ref_root = sys.argv[1]
    sys.modules["cv2"] = types.ModuleType("cv2")
    rng = np.random.default_rng(47)
    cameras, images, points3d = synthetic_model(rng)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        C.write_model(os.path.join(tmp, "model"), cameras, images, points3d)
        for name in ("cameras.bin", "images.bin", "points3D.bin"):
            out["file/sparse/0/" + name] = np.frombuffer(open(os.path.join(tmp, "model", name), "rb").read(), np.uint8)
    for k, im in images.items():
        blocks = np.kron(rng.integers(8, 248, (WH[1] // 4, WH[0] // 4, 3)), np.ones((4, 4, 1), np.int64))
        out["file/images/" + im.name] = file_bytes((blocks + rng.integers(-8, 9, blocks.shape)).astype(np.uint8), "JPEG", quality=90,
                                                   subsampling=0)
        if k % 2:
            mask = np.kron(rng.choice(np.array([0, 254, 255], np.uint8), (WH[1] // 4, WH[0] // 4)), np.ones((4, 4), np.uint8))
            out["file/masks/" + im.name + ".png"] = file_bytes(mask, "PNG")
    out["names"] = np.array([images[k + 1].name for k in range(N_IMAGES)])
    for run, flags in RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            dense = os.path.join(tmp, "colmap_small")
            for key, v in out.items():
                if key.startswith("file/"):
                    os.makedirs(os.path.dirname(os.path.join(dense, key[5:])), exist_ok=True)
                    open(os.path.join(dense, key[5:]), "wb").write(v.tobytes())
            before = {os.path.relpath(os.path.join(d, f), dense) for d, _, fs in os.walk(dense) for f in fs}
            argv = sys.argv
            sys.argv = ["colmap2mvsnet.py", "--dense_folder", dense] + flags
            try:
                runpy.run_path(os.path.join(ref_root, "colmap2mvsnet.py"), run_name="__main__")
            finally:
                sys.argv = argv
            written = sorted({os.path.relpath(os.path.join(d, f), dense) for d, _, fs in os.walk(dense) for f in fs} - before)
            out[f"{run}/written"] = np.array(written)
            for rel in written:
                if rel.endswith(".txt"):
                    out[f"{run}/text/{rel}"] = np.array(open(os.path.join(dense, rel)).read())
                else:                                       # a copy: the name of the file whose bytes it holds
                    data = open(os.path.join(dense, rel), "rb").read()
                    src = [k[5:] for k, v in out.items() if k.startswith("file/") and v.tobytes() == data]
                    assert len(src) == 1, rel
                    out[f"{run}/copy/{rel}"] = np.array(src[0])
            if run == "default":                            # the ranking must not hinge on the digits %f drops
                rows = C.read_pair_text(out["default/text/pair.txt"].item())
                assert all(len(r) == N_IMAGES for r in rows)
                gap = min(float(np.diff(np.sort([s for _, s in r])).min()) for r in rows)
                print("smallest gap between two scores of a row (the diagonal's 0 included):", gap)
                assert gap > 1e-3, gap
    out["flags"] = np.array(repr(RUNS))
    path = os.path.join(HERE, "colmap_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
