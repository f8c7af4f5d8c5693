"""Writes tests/golden/clean_mesh_sphere3.npz and clean_mesh_edges.npz: inputs and recorded results OF THE REFERENCE MODULE
evaluation/clean_mesh.py.  Run only where the reference tree exists:
    python tests/golden/make_golden_clean_mesh.py /path/to/reference

The module needs OpenCV, trimesh, pyembree and open3d, none of which is at hand, so it is loaded with stubs (all in this
harness, none in the reference):
  * ``cv2.imread``: PIL, channels reversed to BGR; ``cv2.getStructuringElement(MORPH_ELLIPSE, (k, k))`` and ``cv2.dilate``:
    the table and the maximum of stage 1 (tests/clean_mesh_ref.py: ``ellipse``, ``dilate``), per channel;
  * ``cv2.decomposeProjectionMatrix``: ``scipy.linalg.rq`` of P[:, :3] with the signs fixed to a positive diagonal of K, and
    the camera centre -inv(P[:, :3]) P[:, 3] as the homogeneous 4x1 vector;
  * ``trimesh``: ``load`` hands back the fixture's arrays, ``Trimesh(v, f).export`` captures what it is given; ``open3d``,
    ``tqdm``: empty (the functions recorded here do not reach them).
One substitution: ``clean_points_by_mask`` hard-codes a 1200 x 1600 image (the literals 1600, 1200, 1202, 1201, 1601).  The
fixtures are 48 x 64, so the module's text is loaded with those five literals replaced by W, H, H + 2, H + 1, W + 1 -- in
memory only; nothing of the reference is written anywhere.

Recorded: ``clean_points_by_mask`` for minimal_vis 0, 1, 2 (three views: together they are the vote count),
``clean_mesh_faces_by_mask`` (the stage-2 mesh, minimal_vis 1), ``load_K_Rt_from_P`` and ``gen_rays_from_single_image`` per
view.  The first-hit and component stages of the reference run on pyembree and trimesh's graph code and cannot be recorded;
the restatement is their specification (include/ufr.h).

Fixtures (3 views, 48 x 64 colour masks whose blue channel is the mask, the other two channels deliberately different):
  sphere3  a 2 208-face latitude-longitude unit sphere seen from three cameras on a radius-3 arc, principal point off-centre
           by (0.37, 0.21); a concentric inner sphere (never hit first); a 300-face blob outside two views' masks (removed by
           the votes); an 80-face island in front of the sphere (removed by min_faces = 100)
  edges    vertices that view 0 projects to px = -1, -2, W-1, W (and the same in y), one behind camera 0, one with q.z = 0,
           over a small grid of ordinary vertices
The generator asserts that every finite pixel coordinate of ``edges`` is at least 1e-6 from a half-integer, and that the close
share of ``sphere3`` (tests/clean_mesh_ref.py) is at most 0.5 %, and prints it."""
import argparse
import contextlib
import io
import os
import re
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clean_mesh_ref as R  # noqa: E402

H, W = 48, 64
SCAN = 24
VIEWS = [23, 24, 33]
MIN_FACES = 100


# ------------------------------------------------------------------ scene
def latlong_sphere(nlat, nlon, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """poles on the y axis; 2 + (nlat - 1) nlon vertices, 2 nlon (nlat - 1) faces, outward winding"""
    v = [(0.0, 1.0, 0.0)]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        for j in range(nlon):
            ph = 2 * np.pi * j / nlon
            v.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    f = []
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon   # noqa: E731
    for j in range(nlon):
        f.append((0, ring(1, j + 1), ring(1, j)))
        f.append((len(v) - 1, ring(nlat - 1, j), ring(nlat - 1, j + 1)))
    for i in range(1, nlat - 1):
        for j in range(nlon):
            f.append((ring(i, j), ring(i, j + 1), ring(i + 1, j)))
            f.append((ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)))
    return np.asarray(v, np.float64) * radius + np.asarray(centre, np.float64), np.asarray(f, np.int32)


def join(parts):
    vs, fs, off = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def cameras(focal=62.0):
    """three (K, E) float32 pairs on a radius-3 arc in the xz plane, looking at the origin (x right, y down, z forward); the
    middle one has exact entries"""
    K = np.array([[focal, 0, W / 2 + 0.37], [0, focal, H / 2 + 0.21], [0, 0, 1]], np.float32)
    cams = []
    for deg in (-25.0, 0.0, 25.0):
        a = np.deg2rad(deg)
        eye = 3.0 * np.array([np.sin(a), 0.0, np.cos(a)])
        fwd = -eye / 3.0
        right = np.array([np.cos(a), 0.0, -np.sin(a)])
        down = np.array([0.0, -1.0, 0.0])
        E = np.eye(4)
        E[:3, :3] = np.stack([right, down, fwd])
        E[:3, 3] = -E[:3, :3] @ eye
        if deg == 0.0:
            E = np.round(E)
            E[2, 3] = 3.0
        cams.append((K.copy(), E.astype(np.float32)))
    return [cams[1], cams[0], cams[2]]          # view 0 is the exact one


def disc_mask(cx, cy, rad):
    ys, xs = np.mgrid[:H, :W]
    return (((xs - cx) ** 2 + (ys - cy) ** 2) <= rad * rad).astype(np.uint8) * 255


# ------------------------------------------------------------------ the reference module under stubs
def load_reference(ref_root):
    import scipy.linalg
    from PIL import Image

    cv = types.ModuleType("cv2")
    cv.MORPH_ELLIPSE = 2
    cv.imread = lambda p: np.ascontiguousarray(np.array(Image.open(p).convert("RGB"), np.uint8)[:, :, ::-1])
    cv.getStructuringElement = lambda shape, ksize: R.ellipse(ksize[0])

    def dilate(img, kernel, iterations=1):
        assert iterations == 1 and np.array_equal(kernel, R.ellipse(kernel.shape[0]))
        return np.stack([R.dilate(img[:, :, c], kernel.shape[0]) for c in range(img.shape[2])], -1)

    def decompose(P):
        P = np.asarray(P, np.float64)
        K, Rm = scipy.linalg.rq(P[:, :3])
        D = np.diag(np.sign(np.diag(K)))
        K, Rm = K @ D, D @ Rm
        assert np.linalg.det(Rm) > 0
        C = -np.linalg.inv(P[:, :3]) @ P[:, 3]
        return K, Rm, np.concatenate([C, [1.0]])[:, None]

    cv.dilate = dilate
    cv.decomposeProjectionMatrix = decompose

    store = {}
    tm = types.ModuleType("trimesh")
    tm.load = lambda p: types.SimpleNamespace(vertices=store[p][0].copy(), faces=store[p][1].astype(np.int64))

    class Trimesh:
        def __init__(self, v, f):
            self.v, self.f = np.asarray(v), np.asarray(f)

        def export(self, p):
            store[p] = (self.v.copy(), self.f.copy())

    tm.Trimesh = Trimesh
    o3d = types.ModuleType("open3d")
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda x, *a, **k: x
    sys.modules.update({"cv2": cv, "trimesh": tm, "open3d": o3d, "tqdm": tq})
    text = open(os.path.join(ref_root, "evaluation", "clean_mesh.py")).read()
    subst = {"1600": W, "1200": H, "1202": H + 2, "1201": H + 1, "1601": W + 1}
    text = re.sub(r"\b(%s)\b" % "|".join(subst), lambda m: str(subst[m.group(1)]), text)      # one pass
    mod = types.ModuleType("reference_clean_mesh")
    exec(compile(text, "reference_clean_mesh", "exec"), mod.__dict__)
    return mod, store


def write_tree(root, cams, masks):
    from PIL import Image

    os.makedirs(os.path.join(root, "cameras"))
    os.makedirs(os.path.join(root, "scan%d" % SCAN, "mask"))
    for vid, (K, E), m in zip(VIEWS, cams, masks):
        with open(os.path.join(root, "cameras", "{:0>8}_cam.txt".format(vid)), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join("%.9g" % x for x in row) for row in E) + "\n\nintrinsic\n"
                    + "\n".join(" ".join("%.9g" % x for x in row) for row in K) + "\n\n0 1\n")
        rgb = np.stack([np.zeros_like(m), 255 - m, m], -1)                 # the mask is the BLUE channel
        Image.fromarray(rgb).save(os.path.join(root, "scan%d" % SCAN, "mask", "{:0>3}.png".format(vid)))


def record(mod, store, name, verts, faces, cams, masks):
    import torch

    out = dict(verts=verts, faces=faces, min_faces=np.int32(MIN_FACES))
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, cams, masks)
        args = argparse.Namespace(root_dir=root)
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):     # the reference prints the mesh
            for k in (0, 1, 2):
                out[f"ref_keep_{k}"] = np.asarray(mod.clean_points_by_mask(args, verts.copy(), SCAN, VIEWS, k, 11))
            store["in.ply"] = (verts, faces)
            mod.clean_mesh_faces_by_mask(args, "in.ply", "out.ply", SCAN, VIEWS, minimal_vis=1, mask_dilated_size=11)
        out["ref_verts2"], out["ref_faces2"] = store["out.ply"][0], store["out.ply"][1].astype(np.int32)
        for i, vid in enumerate(VIEWS):
            K, E = cams[i]
            out[f"K_{i}"], out[f"E_{i}"], out[f"mask_{i}"] = K, E, masks[i]
            P = mod.read_cam_file(os.path.join(root, "cameras", "{:0>8}_cam.txt".format(vid)))
            assert np.array_equal(P, R.projection(K, E)), "the camera file does not round-trip"
            intr, pose = mod.load_K_Rt_from_P(None, P[:3, :])
            out[f"ref_K_{i}"], out[f"ref_pose_{i}"] = intr, pose
            rays = mod.gen_rays_from_single_image(H, W, torch.zeros(3, H, W), torch.from_numpy(intr)[:3, :3].float(),
                                                  torch.from_numpy(pose).float())
            out[f"ref_rays_o_{i}"] = rays["rays_o"][0].numpy()
            out[f"ref_rays_v_{i}"] = rays["rays_v"].numpy()
    path = os.path.join(HERE, f"clean_mesh_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(verts)} vertices, {len(faces)} faces")
    return out


def make_sphere3(mod, store):
    cams = cameras()
    verts, faces = join([latlong_sphere(24, 48), latlong_sphere(12, 24, 0.6), latlong_sphere(11, 15, 0.13, (0.75, 0.7, 1.6)),
                         latlong_sphere(6, 8, 0.12, (0.05, 0.45, 1.2))])
    assert len(faces) == 2208 + 528 + 300 + 80
    masks = [disc_mask(W / 2 + 0.37, H / 2 + 0.21, 24.0) for _ in cams]
    masks[1][:, 50:] = 0                       # the blob lies outside the masks of views 1 and 2
    masks[2][:12, :] = 0
    masks[2][:, 56:] = 0
    record(mod, store, "sphere3", verts, faces, cams, masks)
    r = R.clean_mesh(verts, faces, cams, masks, min_faces=MIN_FACES)
    blob = np.arange(1106 + 266, 1106 + 266 + 152)
    island = np.arange(1106 + 266 + 152, len(verts))
    assert (r["votes"][blob] <= 1).all(), "the blob must lose the vote"
    assert (r["votes"][island] >= 2).all() and (r["votes"][:1106] >= 2).sum() > 600
    f2, f3 = r["faces2"], r["faces3"]
    n_outer = len(R.keep_by_votes(verts, faces[:2208], r["votes"])[1])
    n_inner = len(R.keep_by_votes(verts, faces[2208:2736], r["votes"])[1])
    hit_idx = set(np.concatenate([i[i >= 0] for i in r["face_ids"]]).tolist())
    assert not any(n_outer <= i < n_outer + n_inner for i in hit_idx), "the inner sphere must never be hit first"
    assert any(i >= n_outer + n_inner for i in hit_idx), "the island must be visible"
    assert len(r["faces"]) >= 500 and r["faces"].max() < (r["votes"][:1106] >= 2).sum(), "only the outer sphere survives"
    n_close = sum(int(c.sum()) for c in r["close"])
    n_rays = sum(int(m.sum()) for m in r["dilated"])
    print(f"sphere3: {n_close} close pixels of {n_rays} rays ({100.0 * n_close / n_rays:.3f} %); stage 2: {len(f2)} faces, "
          f"first hit: {len(f3)}, final: {len(r['faces'])} faces in components of >= {MIN_FACES}")
    assert n_close <= 0.005 * n_rays


def make_edges(mod, store):
    cams = cameras()
    K, E = [c.astype(np.float64) for c in cams[0]]
    Kinv, c2w = np.linalg.inv(K), np.linalg.inv(E)

    def back(px, py, depth):
        return (c2w @ np.append(Kinv @ np.array([px, py, 1.0]) * depth, 1.0))[:3]

    special = [back(-1.3, 20.2, 3.0), back(-2.2, 20.2, 3.0), back(W - 1 + 0.3, 20.2, 3.0), back(W + 0.2, 20.2, 3.0),
               back(30.3, -1.3, 3.0), back(30.3, -2.2, 3.0), back(30.3, H - 1 + 0.3, 3.0), back(30.3, H + 0.2, 3.0),
               back(-0.7, -0.8, 2.5), back(W - 0.7, H - 0.8, 2.5),
               back(30.3, 20.2, -1.5),                      # behind camera 0, projecting inside the image: it counts
               np.array([0.21, -0.13, 3.0])]                # q.z = -z + 3 = 0 in view 0
    grid = [np.array([x, y, 0.1 * x * y]) for y in np.linspace(-0.9, 0.9, 7) + 0.013 for x in np.linspace(-1.2, 1.2, 9) + 0.007]
    verts = np.asarray(grid + special, np.float64)
    ng = len(grid)
    faces = []
    for j in range(6):
        for i in range(8):
            a = j * 9 + i
            faces += [(a, a + 1, a + 9), (a + 1, a + 10, a + 9)]
    for s in range(len(special)):
        faces.append((ng + s, (7 * s) % ng, (7 * s + 1) % ng))
        faces.append((ng + s, ng + (s + 1) % len(special), (5 * s) % ng))
    faces = np.asarray(faces, np.int32)
    masks = [disc_mask(30.0, 22.0, 40.0), disc_mask(28.0, 24.0, 19.0), disc_mask(36.0, 20.0, 17.0)]
    masks[0][:, :3] = 0
    masks[0][:, W - 1] = 0                       # the dilation refills it: the column W-1 is read, and set
    # every finite pixel coordinate at least 1e-6 from a half-integer
    for Kc, Ec in cams:
        P = R.projection(Kc, Ec).astype(np.float64)
        q = verts @ P[:3, :3].T + P[:3, 3]
        with np.errstate(all="ignore"):
            uv = q[:, :2] / q[:, 2:]
        uv = uv[np.isfinite(uv)]
        assert (np.abs(uv - np.floor(uv) - 0.5) >= 1e-6).all()
    P0 = R.projection(*cams[0]).astype(np.float64)
    assert (P0[2, :3] @ verts[-1] + P0[2, 3]) == 0.0 and (P0[2, :3] @ verts[-2] + P0[2, 3]) < 0
    out = record(mod, store, "edges", verts, faces, cams, masks)
    votes = out["ref_keep_0"].astype(int) + out["ref_keep_1"] + out["ref_keep_2"]
    dil0 = R.dilated_mask(masks[0])
    rx = np.rint((verts[ng:ng + 4] @ P0[:3, :3].T + P0[:3, 3])[:, 0] / 3.0)
    assert rx.tolist() == [-1, -2, W - 1, W] and dil0[20, W - 1]
    print("edges: votes of the special vertices", votes[ng:].tolist(), "stage-2 faces", len(out["ref_faces2"]))


if __name__ == "__main__":
    ref_root = sys.argv[1]
    mod, store = load_reference(ref_root)
    make_sphere3(mod, store)
    make_edges(mod, store)
