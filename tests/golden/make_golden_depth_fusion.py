"""Writes tests/golden/depth_fusion_full.npz and depth_fusion_nview.npz: inputs and recorded results OF THE REFERENCE MODULE
code1/encoder_utils/depth_fusion.py, imported unmodified.  Run only where the reference tree exists:
    python tests/golden/make_golden_depth_fusion.py /path/to/reference

Two stubs, both in this harness and none in the reference:
  * ``cv2``: ``remap`` is the numpy restatement tests/depth_fusion_ref.py documents (no OpenCV is a dependency here, so the
    recorded run pins everything BUT the bilinear lookup to the reference);
  * ``plyfile``: ``PlyElement.describe`` and ``PlyData.write`` capture the structured vertex array instead of writing it.
The reference's ``filter_depth`` runs on a temporary tree of ``depth/<scan>/<%08d>.npy`` dicts, ``rgb/<scan>/<%08d>.jpg`` and
``pair.txt``: once with --full_fusion on a pair file with unequal source counts (2, 1, 3, 0 -- dropped by the reader --, 10, 1;
with six views the ten sources repeat views, the reference view itself among them), once without (n_view 3).  The locals of
``filter_depth`` (geo_mask_sum, depth_est_averaged) are read off its frame when it calls ``save_mask``; the masks are the PNGs
it wrote.  ``reproject_with_depth`` is then called for every pair to record ``dist`` and ``relative_depth_diff``, the margins
the GPU test's near-threshold exemption is defined on.

The cameras are float64: float32 intrinsics / extrinsics go through LAPACK's float32 inverse, whose last bit differs between
BLAS kernels, and a fixture must give the same bits on every host.  (float32 cameras, what the model writes, are covered
by the GPU tests against the restatement, both fed by the same host's inverses.)

Only data is stored: inputs (depths, cameras, decoded colours, pairs, thresholds), masks (packbits), geo_mask_sum,
depth_est_averaged at the valid pixels, vertices, colours, and the margins as float32."""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import depth_fusion_ref as R  # noqa: E402

SCAN = "scan9"


# ------------------------------------------------------------------ the scene: a sphere in front of a plane
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """world-to-camera 4x4 (x right, y down, z forward)"""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    E = np.eye(4)
    E[:3, :3] = np.stack([r, d, f])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def render_depth(K, E, h, w, radius=0.3, plane_z=-0.4):
    """z-depth of the nearer of a sphere at the origin and the plane z = plane_z, per pixel centre"""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])          # camera space, z = 1
    Rm, t = E[:3, :3], E[:3, 3]
    o = -Rm.T @ t
    d = Rm.T @ rays
    tp = (plane_z - o[2]) / d[2]
    tp = np.where(tp > 0, tp, np.inf)
    b = (d * o[:, None]).sum(0)
    a = (d * d).sum(0)
    disc = b * b - a * (o @ o - radius * radius)
    ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    z = np.minimum(tp, ts)                                                                 # rays have z = 1: t IS the z-depth
    assert np.isfinite(z).all(), "the scene must cover the whole image"
    return z.reshape(h, w)


def make_views(seed=0):
    rng = np.random.default_rng(seed)
    H, W = 60, 80
    eyes = [(0.0, 0.3, 6.0), (0.3, 0.2, 6.0), (-2.5, -0.4, 5.5), (3.2, 0.9, 5.0), (-0.5, 2.0, 5.8), (0.2, -0.6, 6.0)]
    targets = [(0.0, 0.0, 0.0), (0.12, 0.05, 0.0), (-0.1, -0.08, 0.0), (0.2, 0.1, 0.0), (-0.05, 0.12, 0.0), (0.0, 0.0, 0.0)]
    depths, Ks, Es, colors = [], [], [], []
    for v, (eye, tgt) in enumerate(zip(eyes, targets)):
        h, w = (40, 56) if v == 4 else (H, W)                   # one view of another size, with its own intrinsics
        f = 7.0 * w
        K = np.array([[f, 0.0, (w - 1) / 2 + 0.7], [0.0, f * 1.01, (h - 1) / 2 - 0.4], [0.0, 0.0, 1.0]])
        E = look_at(eye, tgt)
        z = render_depth(K, E, h, w)
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        z = z * (1 + 0.006 * np.sin(xs / 6.0 + v) * np.cos(ys / 5.0 - v))                          # smooth error
        z = z * (1 + np.where(rng.random((h, w)) < 0.35, 0.012 * rng.standard_normal((h, w)), 0))   # pixel-level error
        z[rng.random((h, w)) < 0.035] = 0                                                           # holes
        z[5:9, 11:17] = 0
        if v == 5:
            z[:] = 0                                                                                # a view without depth
        depths.append(z.astype(np.float32))
        Ks.append(K)
        Es.append(E)
        colors.append(np.stack([xs * 255 // w, ys * 255 // h, (xs + ys + 16 * v) % 256], -1).astype(np.uint8))   # smooth: the JPEG keeps it small
    return depths, Ks, Es, colors


FULL_PAIRS = [(0, [1, 2]), (1, [0]), (2, [0, 3, 4]), (3, []), (4, [0, 1, 2, 3, 5, 2, 1, 3, 4, 0]), (5, [0])]


def write_tree(root, dataset, depths, Ks, Es, colors):
    from PIL import Image

    os.makedirs(os.path.join(root, "depth", SCAN))
    os.makedirs(os.path.join(root, "rgb", SCAN))
    os.makedirs(os.path.join(root, SCAN))
    os.makedirs(os.path.join(root, "pcd"))
    decoded = []
    for v, (d, K, E, c) in enumerate(zip(depths, Ks, Es, colors)):
        np.save(os.path.join(root, "depth", SCAN, "%08d.npy" % v), {"depth": d, "extrinsic": E, "intrinsic": K})
        p = os.path.join(root, "rgb", SCAN, "%08d.jpg" % v)
        Image.fromarray(c).save(p)
        decoded.append(np.array(Image.open(p), dtype=np.uint8))
    with open(os.path.join(dataset, "pair.txt"), "w") as f:
        f.write("%d\n" % len(FULL_PAIRS))
        for ref, srcs in FULL_PAIRS:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d %.3f" % (s, 100.0 - k) for k, s in enumerate(srcs))))
    return decoded


# ------------------------------------------------------------------ the reference module behind its two stubs
def load_reference(ref_root, captured):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1
    cv2.remap = lambda src, x, y, interpolation=None: R.remap(src, x, y)

    plyfile = types.ModuleType("plyfile")

    class PlyElement:
        @staticmethod
        def describe(data, name):
            return (name, data)

    class PlyData:
        def __init__(self, elements):
            self.elements = elements

        def write(self, filename):
            (name, data), = self.elements
            assert name == "vertex"
            captured["ply"] = (filename, data.copy())

    plyfile.PlyElement, plyfile.PlyData = PlyElement, PlyData
    sys.modules["cv2"], sys.modules["plyfile"] = cv2, plyfile
    spec = importlib.util.spec_from_file_location("reference_depth_fusion",
                                                  os.path.join(ref_root, "code1", "encoder_utils", "depth_fusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    save_mask = mod.save_mask

    def recording_save_mask(filename, mask):          # filter_depth's locals at the moment it saves a view's mask
        loc = sys._getframe(1).f_locals
        captured.setdefault("views", []).append(dict(ref=int(loc["ref_view"]), geo_mask_sum=np.array(loc["geo_mask_sum"]),
                                                     depth_est_averaged=np.array(loc["depth_est_averaged"])))
        save_mask(filename, mask)

    mod.save_mask = recording_save_mask
    return mod


def run(mod, captured, root, dataset, views, pairs, args):
    from PIL import Image

    depths, Ks, Es, colors = views
    captured.clear()
    mod.filter_depth(argparse.Namespace(root_dir=root, dataset_dir=dataset, **args), SCAN)
    pt, dt, mt = args["geo_pixel_thres"], args["geo_depth_thres"], args["geo_mask_thres"]
    out = dict(geo_pixel_thres=np.float64(pt), geo_depth_thres=np.float64(dt), geo_mask_thres=np.int32(mt),
               n_views=np.int32(len(depths)), full_fusion=np.int32(args["full_fusion"]), n_view=np.int32(args["n_view"]),
               pair_ref=np.array([r for r, _ in pairs], np.int32), pair_len=np.array([len(s) for _, s in pairs], np.int32),
               pair_src=np.array([s for _, ss in pairs for s in ss], np.int32))
    for v in range(len(depths)):
        out[f"depth_{v}"], out[f"K_{v}"], out[f"E_{v}"], out[f"color_{v}"] = depths[v], Ks[v], Es[v], colors[v]
    assert [c["ref"] for c in captured["views"]] == [r for r, _ in pairs]
    stats = dict(n=0, pix_only=0, depth_only=0, outside=0, partial=0, close=0, zero_ref=0, ref_px=0, kept=0)
    zero_valid = False
    for i, ((ref, srcs), c) in enumerate(zip(pairs, captured["views"])):
        mask = np.array(Image.open(os.path.join(root, SCAN, "mask", "%08d.png" % ref))) > 0
        assert np.array_equal(mask, c["geo_mask_sum"] >= mt)
        out[f"mask_{i}"] = np.packbits(mask)
        out[f"geo_mask_sum_{i}"] = c["geo_mask_sum"].astype(np.int32)
        assert c["depth_est_averaged"].dtype == np.float64
        out[f"depth_avg_valid_{i}"] = c["depth_est_averaged"][mask]
        zero_valid |= not mask.any()
        stats["ref_px"] += mask.size
        stats["kept"] += int(mask.sum())
        stats["zero_ref"] += int((depths[ref] == 0).sum())
        h, w = depths[ref].shape
        xg, yg = np.meshgrid(np.arange(0, w), np.arange(0, h))
        dist_all, rel_all = [], []
        for s in srcs:
            drep, xr, yr, xs, ys = mod.reproject_with_depth(depths[ref], Ks[ref], Es[ref], depths[s], Ks[s], Es[s])
            with np.errstate(all="ignore"):
                dist = np.sqrt((xr - xg) ** 2 + (yr - yg) ** 2)
                rel = np.abs(drep - depths[ref]) / depths[ref]
            dist_all.append(dist.astype(np.float32))
            rel_all.append(rel.astype(np.float32))
            nz = depths[ref] != 0
            outside = R.taps_outside(depths[s].shape, xs, ys)
            on_zero = R.remap((depths[s] == 0).astype(np.float32), xs, ys) > 0
            with np.errstate(invalid="ignore"):
                stats["n"] += int(nz.sum())
                stats["pix_only"] += int((nz & ~(dist < pt) & (rel < np.float32(dt))).sum())
                stats["depth_only"] += int((nz & (dist < pt) & ~(rel < np.float32(dt))).sum())
                stats["outside"] += int((nz & (outside == 4)).sum())
                stats["partial"] += int((nz & (((outside > 0) & (outside < 4)) | ((outside < 4) & on_zero))).sum())
                stats["close"] += int((nz & R.close_pairs(dist, rel, pt, dt)).sum())
        out[f"dist_{i}"] = np.stack(dist_all)
        out[f"rel_{i}"] = np.stack(rel_all)
    filename, ply = captured["ply"]
    assert filename == os.path.join(root, "pcd", SCAN + ".ply")
    out["verts"] = np.stack([ply["x"], ply["y"], ply["z"]], 1)
    out["vert_colors"] = np.stack([ply["red"], ply["green"], ply["blue"]], 1)
    assert out["verts"].dtype == np.float32 and out["vert_colors"].dtype == np.uint8 and len(out["verts"]) == stats["kept"]
    return out, stats, zero_valid


def check_coverage(stats, zero_valid, different_sizes):
    """every branch does work on the reference's own record"""
    n = stats["n"]
    share = {k: stats[k] / n for k in ("pix_only", "depth_only", "outside", "partial", "close")}
    share["zero_ref"] = stats["zero_ref"] / stats["ref_px"]
    share["kept"] = stats["kept"] / stats["ref_px"]
    print({k: round(v, 4) for k, v in share.items()}, "pairs x pixels:", n)
    assert share["pix_only"] >= 0.02 and share["depth_only"] >= 0.02 and share["outside"] >= 0.02 and share["partial"] >= 0.02, share
    assert share["zero_ref"] >= 0.02 and 0.10 <= share["kept"] <= 0.90, share
    assert share["close"] <= 0.005, share
    assert zero_valid, "no reference view ends with zero valid pixels"
    assert different_sizes, "no pair joins views of different sizes"


def main():
    ref_root = sys.argv[1]
    captured = {}
    mod = load_reference(ref_root, captured)
    depths, Ks, Es, colors = make_views()
    with tempfile.TemporaryDirectory() as tmp:
        root, dataset = os.path.join(tmp, "out"), os.path.join(tmp, "dataset")
        os.makedirs(root)
        os.makedirs(dataset)
        decoded = write_tree(root, dataset, depths, Ks, Es, colors)
        views = (depths, Ks, Es, decoded)
        runs = {
            "full": (mod.read_pair_file(os.path.join(dataset, "pair.txt")),
                     dict(n_view=3, geo_pixel_thres=1, geo_depth_thres=0.01, geo_mask_thres=2, full_fusion=True)),
            "nview": ([(0, [1, 2]), (1, [0, 2]), (2, [0, 1])],
                      dict(n_view=3, geo_pixel_thres=0.5, geo_depth_thres=0.005, geo_mask_thres=1, full_fusion=False)),
        }
        assert runs["full"][0] == [(r, s) for r, s in FULL_PAIRS if s]
        for name, (pairs, args) in runs.items():
            out, stats, zero_valid = run(mod, captured, root, dataset, views, pairs, args)
            sizes = any(depths[r].shape != depths[s].shape for r, ss in pairs for s in ss)
            if name == "full":                     # the whole coverage list is asserted on the full run
                check_coverage(stats, zero_valid, sizes)
            else:
                print({k: round(stats[k] / stats["n"], 4) for k in ("pix_only", "depth_only", "outside", "partial", "close")})
                assert stats["close"] / stats["n"] <= 0.005
            path = os.path.join(HERE, f"depth_fusion_{name}.npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "bytes;", len(out["verts"]), "points")


if __name__ == "__main__":
    main()
