"""The rendering kernels (csrc/raster.hip, and csrc/mesh_clean.hip's first hit without a mask) against the numpy restatement
(raster_ref.py), on tests/golden/clean_mesh_sphere3.npz (3 116 faces, 48 x 64, read-only) and small hand-made meshes.

uint8 images: exact on every pixel that is not *close* by the restatement's own margins (raster_ref.py), at most one level on the
close ones, and the close share of an image is at most 0.5 % (the five path frames used here have none at all: checked with
the restatement alone).  Face ids are equal off close pixels.  Depth: both sides form t * v.z in float64 and narrow once, so
within 1 float32 ulp.  Normal maps: within 1e-6.  Vertex normals: the same float64 expressions without contraction, so each
component within 1e-14 (a few ulp of values <= 1), and two runs give the same bits."""
import ctypes as C
import os

import numpy as np
import pytest

import clean_mesh_ref as R
import raster_ref as RR
from test_clean_mesh import latlong_sphere
from test_render_trajectory import EXACT_K, tie_image
from uforecon_amd import _lib, clean_mesh as CM, dtu_eval, ops, render_trajectory as RT
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 48, 64
FRAMES = [0, 60, 119, 120, 239]
CLOSE_CAP = 0.005


def cuda(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


_scene = {}


def scene():
    """the fixture's mesh, the five frames of the path through its three cameras and the restatement's renders of them,
    computed once and shared (never modified)"""
    if not _scene:
        g = np.load(os.path.join(HERE, "golden", "clean_mesh_sphere3.npz"))
        v, f = g["verts"].astype(np.float64), g["faces"].astype(np.int32)
        w2cs = np.stack([g[f"E_{i}"].astype(np.float64) for i in range(3)])
        c2ws = RT.interpolate_trajectory(w2cs, 240)[FRAMES]
        K = g["K_0"]
        k_inv = CM.ray_camera(K, np.eye(4, dtype=np.float32))[0]
        normals = RR.vertex_normals(v, f)
        colors = np.random.default_rng(5).integers(0, 256, (len(v), 3)).astype(np.uint8)
        smooth, flat = [], []
        for c in c2ws.astype(np.float32):
            hit = R.first_hit(v, f, k_inv, c, np.ones((H, W), bool), return_close=True)
            smooth.append(RR.render(v, f, k_inv, c, H, W, normals=normals, hit=hit))
            flat.append(RR.render(v, f, k_inv, c, H, W, colors=colors, hit=hit))
        _scene.update(v=v, f=f, K=K, k_inv=k_inv, c2ws=c2ws, normals=normals, colors=colors, smooth=smooth, flat=flat)
    return _scene


def assert_render_agrees(got, want, maps=True):
    """got: (image, depth, normal, face_id) of one frame from the GPU; want: raster_ref.render's dict"""
    image, depth, normal, face_id = got
    close = want["close"]
    share = close.mean()
    diff = np.abs(image.astype(np.int32) - want["image"].astype(np.int32)).max(-1)
    print(f"close share {share:.4f}, image diff max {diff.max()}, off close {diff[~close].max() if (~close).any() else 0}")
    assert share <= CLOSE_CAP
    assert (diff[~close] == 0).all() and (diff <= 1).all()
    if maps:
        assert np.array_equal(face_id[~close], want["face_id"][~close])
        ulp = np.spacing(np.abs(want["depth"]).astype(np.float32))
        derr = np.abs(depth.astype(np.float64) - want["depth"].astype(np.float64))
        nerr = np.abs(normal.astype(np.float64) - want["normal"].astype(np.float64)).max()
        print(f"depth err max {derr.max():.3g} (ulp {ulp.max():.3g}), normal err max {nerr:.3g}")
        assert (derr <= ulp).all() and nerr <= 1e-6


def gpu_normals(v, f):
    return ops.raster_vertex_normals(cuda(np.asarray(v, np.float64)), cuda(np.asarray(f, np.int32).reshape(-1, 3)))


# ------------------------------------------------------------------ vertex normals
def test_vertex_normals_on_sphere3_match_and_repeat():
    s = scene()
    a, b = gpu_normals(s["v"], s["f"]).cpu().numpy(), gpu_normals(s["v"], s["f"]).cpu().numpy()
    err = np.abs(a - s["normals"]).max()
    print("vertex normal err", err)
    assert a.dtype == np.float64 and err <= 1e-14
    assert a.tobytes() == b.tobytes()


def test_vertex_normals_long_run_and_crowded_block():
    """a 1 000-face fan round vertex 0 (a run longer than a workgroup) beside a sphere whose vertex count is no multiple of 256"""
    ang = 2 * np.pi * np.arange(1000) / 1000
    rim = np.stack([np.cos(ang), np.sin(ang), 0.3 * np.sin(5 * ang)], 1)
    fan_v = np.concatenate([[[0.0, 0.0, 0.5]], rim])
    fan_f = np.stack([np.zeros(1000, np.int64), 1 + np.arange(1000), 1 + (np.arange(1000) + 1) % 1000], 1)
    sv, sf = latlong_sphere(20, 27, radius=0.7, centre=(3.0, 0.0, 0.0))
    v = np.concatenate([fan_v, sv])
    f = np.concatenate([fan_f, sf + len(fan_v)]).astype(np.int32)
    assert len(v) % 256 != 0 and len(v) > 1024
    got = gpu_normals(v, f).cpu().numpy()
    assert np.abs(got - RR.vertex_normals(v, f)).max() <= 1e-14
    assert abs(np.linalg.norm(got[0]) - 1) <= 1e-14


def test_vertex_normals_excluded_faces():
    import torch

    sv, sf = latlong_sphere(6, 7)
    v = np.concatenate([sv, [[9.0, 9.0, 9.0]]])                               # an unused vertex
    f = np.concatenate([sf, [[0, 0, 1]]]).astype(np.int32)                    # a zero-area face
    want = RR.vertex_normals(v, f)
    got = gpu_normals(v, f).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-14 and np.array_equal(got[-1], [0, 0, 0])
    assert np.abs(want - np.concatenate([RR.vertex_normals(sv, sf), [[0, 0, 0]]])).max() == 0
    bad = np.concatenate([f, [[1, 2, len(v) + 3]], [[-1, 3, 4]]]).astype(np.int32)   # indices out of range
    with pytest.raises(UfrError):
        gpu_normals(v, bad)
    # the ABI call leaves such faces out
    tv, tf = cuda(v), cuda(bad)
    svert, slots = torch.sort(tf.reshape(-1).to(torch.int64), stable=True)
    runs = torch.searchsorted(svert, torch.arange(len(v) + 1, dtype=torch.int64, device="cuda")).contiguous()
    out = torch.full((len(v), 3), 7.0, dtype=torch.float64, device="cuda")
    rc = _lib.load().ufr_raster_vertex_normals(tv.data_ptr(), tf.data_ptr(), len(v), len(bad), slots.contiguous().data_ptr(),
                                               runs.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-14 and np.abs(RR.vertex_normals(v, bad) - want).max() == 0


# ------------------------------------------------------------------ frames
def render_gpu(v, f, K, c2ws, h, w, **kw):
    return RT.render_mesh(v, f, K, c2ws, h, w, return_depth=True, return_normals=True, return_face_ids=True, **kw)


def test_five_frames_in_one_call_smooth_uniform_and_flat_vertex_colours():
    s = scene()
    smooth = render_gpu(s["v"], s["f"], s["K"], s["c2ws"], H, W)
    flat = render_gpu(s["v"], s["f"], s["K"], s["c2ws"], H, W, colors=s["colors"], smooth=False)
    assert smooth[0].shape == (5, H, W, 3) and smooth[0].dtype == np.uint8 and smooth[1].shape == (5, H, W)
    assert smooth[2].shape == (5, H, W, 3) and smooth[3].dtype == np.int32
    for i in range(5):
        assert_render_agrees([m[i] for m in smooth], s["smooth"][i])
        assert_render_agrees([m[i] for m in flat], s["flat"][i])
        assert (smooth[3][i] >= 0).sum() > 1000 and not np.array_equal(smooth[0][i], flat[0][i])
    # a frame of the batch is the frame rendered alone, bit for bit (a key image left over from the frame before would show)
    for i in range(5):
        for batch, kw in ((smooth, {}), (flat, dict(colors=s["colors"], smooth=False))):
            alone = render_gpu(s["v"], s["f"], s["K"], s["c2ws"][i], H, W, **kw)
            for a, b in zip(alone, batch):
                assert a[0].tobytes() == b[i].tobytes()
    assert not np.array_equal(smooth[3][0], smooth[3][1])


@pytest.mark.parametrize("h,w", [(37, 53), (1, 1)])
def test_sizes_that_do_not_fill_a_block(h, w):
    v, f = latlong_sphere(10, 13)
    K = np.array([[40, 0, (w - 1) / 2], [0, 40, (h - 1) / 2], [0, 0, 1]], np.float32)
    E = np.array([[1, 0, 0, 0.1], [0, -1, 0, 0.05], [0, 0, -1, 3], [0, 0, 0, 1]], np.float32)
    k_inv, c2w = CM.ray_camera(K, E)
    n = RR.vertex_normals(v, f)
    got = render_gpu(v, f, K, c2w, h, w)
    assert got[0].shape == (1, h, w, 3)
    assert_render_agrees([m[0] for m in got], RR.render(v, f, k_inv, c2w, h, w, normals=n))
    assert (got[3] >= 0).any()


def test_camera_inside_the_sphere():
    """from the centre every triangle has a vertex behind the camera or fills a large box: the whole-image path of the first
    hit runs, every pixel is hit, and the faces seen from behind are lit like faces seen from the front"""
    v, f = latlong_sphere(10, 13)
    K = np.array([[20, 0, 26], [0, 20, 18], [0, 0, 1]], np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = [0.05, -0.02, 0.03]
    k_inv = CM.ray_camera(K, np.eye(4, dtype=np.float32))[0]
    for faces in (f, f[:, ::-1].copy()):
        got = render_gpu(v, faces, K, c2w, 37, 53, smooth=False)
        assert_render_agrees([m[0] for m in got], RR.render(v, faces, k_inv, c2w, 37, 53))
        assert (got[3] >= 0).all() and got[0].min() >= 200 and (got[1] > 0).all()
        assert (got[2][0, ..., 2] < 0).all()                                  # camera-space normals face the camera


def test_coincident_triangles_fall_back_to_the_flat_normal():
    v = np.array([[-4.0, -4.0, 8.0], [4.0, -4.0, 8.0], [0.0, 4.0, 8.0]])     # small integers: the two face normals cancel exactly
    f = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    assert np.array_equal(gpu_normals(v, f).cpu().numpy(), np.zeros((3, 3)))
    smooth = render_gpu(v, f, EXACT_K, np.eye(4), H, W)
    flat = render_gpu(v, f, EXACT_K, np.eye(4), H, W, smooth=False)
    for a, b in zip(smooth, flat):
        assert a.tobytes() == b.tobytes()
    hit = smooth[3][0] >= 0
    assert hit.sum() > 50 and (smooth[3][0][hit] == 0).all()                  # the tie in t goes to the lower face
    assert tuple(smooth[0][0, 24, 32]) == (255, 255, 255) and smooth[1][0, 24, 32] == 8.0
    # (every hit pixel is close by the restatement's margins -- two hits at one t, a zero smooth normal -- but the kernel's
    # choices are fixed by rule, so the restatement's must be the same)
    k_inv = R.k_inverse(EXACT_K.astype(np.float64))
    want = RR.render(v, f, k_inv, np.eye(4, dtype=np.float32), H, W, normals=np.zeros((3, 3)))
    assert want["close"][hit].all() and np.array_equal(want["face_id"], smooth[3][0]) and np.array_equal(want["image"], smooth[0][0])


# ------------------------------------------------------------------ downsample
@pytest.mark.parametrize("s", [2, 3])
def test_supersampled_render_equals_the_restatement(s):
    v, f = latlong_sphere(10, 13)
    h, w = 37, 53
    K = np.array([[40, 0, 26], [0, 40, 18], [0, 0, 1]], np.float32)
    E = np.array([[1, 0, 0, 0.1], [0, -1, 0, 0.05], [0, 0, -1, 3], [0, 0, 0, 1]], np.float32)
    _, c2w = CM.ray_camera(K, E)
    k_inv = CM.ray_camera(RT.supersampled_intrinsics(K, s).astype(np.float32), np.eye(4, dtype=np.float32))[0]
    big = RR.render(v, f, k_inv, c2w, s * h, s * w, normals=RR.vertex_normals(v, f))
    assert big["close"].mean() <= CLOSE_CAP
    want = RR.downsample(big["image"][None], s)[0]
    got = RT.render_mesh(v, f, K, c2w, h, w, supersample=s)[0]
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32)).max(-1)
    touched = big["close"].reshape(h, s, w, s).any((1, 3))                    # a small pixel with a close big pixel under it
    assert (diff[~touched] == 0).all() and (diff <= 1).all()
    # the big image itself, then the kernel alone on it
    full = RT.render_mesh(v, f, RT.supersampled_intrinsics(K, s), c2w, s * h, s * w)
    assert np.array_equal(ops.raster_downsample(cuda(full), s).cpu().numpy()[0], got)
    assert np.array_equal(got, RR.downsample(full, s)[0])
    with pytest.raises(UfrError):
        RT.render_mesh(v, f, K, c2w, h, w, supersample=s, return_depth=True)


def test_downsample_ties_and_identity():
    img, want = tie_image()
    out = ops.raster_downsample(cuda(img), 2).cpu().numpy()
    assert out.shape == (1, 1, 6, 3) and all(np.array_equal(out[0, 0, :, c], want) for c in range(3))
    rnd = np.random.default_rng(3).integers(0, 256, (3, 24, 36, 3)).astype(np.uint8)
    for s in (1, 2, 3, 4):
        assert np.array_equal(ops.raster_downsample(cuda(rnd), s).cpu().numpy(), RR.downsample(rnd, s))
    assert np.array_equal(ops.raster_downsample(cuda(rnd), 1).cpu().numpy(), rnd)
    with pytest.raises(UfrError):
        ops.raster_downsample(cuda(rnd), 5)


# ------------------------------------------------------------------ argument errors
def test_abi_rejects_bad_arguments():
    import torch

    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    kinv = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    c2w = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
    assert lib.ufr_raster_vertex_normals(None, None, 1, 1, None, None, None, None) == -1 and b"null" in lib.ufr_last_error()
    assert lib.ufr_raster_vertex_normals(p, p, 0, 1, p, p, p, None) == -1
    assert lib.ufr_raster_vertex_normals(p, p, 1, 2 ** 30, p, p, p, None) == -1
    assert lib.ufr_raster_frames_workspace_bytes(0, 4, 4) == 0 and lib.ufr_raster_frames_workspace_bytes(1, 0, 4) == 0
    assert lib.ufr_raster_frames_workspace_bytes(1, 2 ** 16, 2 ** 15) == 0
    need = lib.ufr_raster_frames_workspace_bytes(10, 48, 64)
    assert need >= 48 * 64 * 12 + 44

    def frames(verts=p, faces=p, ki=kinv, cw=c2w, n=1, h=4, w=4, ambient=0.25, image=p, ws=p, ws_bytes=1 << 16, base=None):
        return lib.ufr_raster_frames(verts, faces, 1, 1, None, None, C.cast(ki, fp), C.cast(cw, fp), n, h, w, base, None, ambient,
                                     image, None, None, None, ws, ws_bytes, None)

    for kw in (dict(verts=None), dict(faces=None), dict(ki=None), dict(cw=None), dict(image=None), dict(ws=None)):
        assert frames(**kw) == -1 and b"null" in lib.ufr_last_error(), kw
    for kw in (dict(n=0), dict(h=0), dict(w=0), dict(h=2 ** 16, w=2 ** 15), dict(ambient=-0.1), dict(ambient=1.5),
               dict(ambient=float("nan")), dict(ws_bytes=64), dict(base=(C.c_float * 3)(0.5, 2.0, 0.5)),
               dict(cw=(C.c_float * 16)(*([0.0] * 16)))):
        assert frames(**kw) == -1 and lib.ufr_last_error(), kw
    assert frames(ws_bytes=64) == -1 and b"workspace" in lib.ufr_last_error()
    assert lib.ufr_raster_downsample(None, 1, 4, 4, 2, None, None) == -1 and b"null" in lib.ufr_last_error()
    for n, h, w, s in ((0, 4, 4, 2), (1, 0, 4, 2), (1, 4, 0, 2), (1, 4, 4, 0), (1, 4, 4, 5), (1, 2 ** 15, 2 ** 15, 2)):
        assert lib.ufr_raster_downsample(p, n, h, w, s, p, None) == -1, (n, h, w, s)
    torch.cuda.synchronize()                                                 # nothing was launched, nothing faulted
    assert int(buf.sum()) == 0


def test_ops_reject_bad_arguments():
    s = scene()
    tv, tf = cuda(s["v"]), cuda(s["f"])
    with pytest.raises(UfrError):
        ops.raster_frames(tv, tf, s["k_inv"], s["c2ws"][:1], H, W, ambient=1.5)
    with pytest.raises(UfrError):
        ops.raster_frames(tv, tf, s["k_inv"], s["c2ws"][:1], 0, W)
    with pytest.raises(UfrError):
        ops.raster_frames(tv, tf, s["k_inv"], s["c2ws"][0, :3], H, W)
    with pytest.raises(UfrError):
        ops.raster_frames(tv, cuda(s["f"] + 5), s["k_inv"], s["c2ws"][:1], H, W)
    with pytest.raises(UfrError):
        ops.raster_frames(tv, tf, s["k_inv"], s["c2ws"][:1], H, W, normals=cuda(s["normals"][:-1]))
    with pytest.raises(UfrError):
        RT.render_mesh(s["v"], s["f"] + 5, s["K"], s["c2ws"][:1], H, W)
    empty = RT.render_mesh(s["v"], np.zeros((0, 3), np.int32), s["K"], s["c2ws"][:2], H, W, background=(1, 2, 3))
    assert empty.shape == (2, H, W, 3) and (empty == np.array([1, 2, 3], np.uint8)).all()


# ------------------------------------------------------------------ the command line
def test_command_line_end_to_end(tmp_path):
    from PIL import Image

    s = scene()
    g = np.load(os.path.join(HERE, "golden", "clean_mesh_sphere3.npz"))
    os.makedirs(tmp_path / "cameras")
    os.makedirs(tmp_path / "mesh")
    for view, i in ((23, 0), (24, 1)):
        with open(tmp_path / "cameras" / "{:0>8}_cam.txt".format(view), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join("%.9g" % x for x in row) for row in g[f"E_{i}"]) + "\n\nintrinsic\n"
                    + "\n".join(" ".join("%.9g" % x for x in row) for row in g[f"K_{i}"]) + "\n\n0 1\n")
    sv, sf = latlong_sphere(10, 13, radius=0.8)
    meshes = {1: (s["v"], s["f"]), 2: (sv, sf)}
    for scan, (v, f) in meshes.items():
        CM.write_ply(str(tmp_path / "mesh" / f"scan{scan}.ply"), v, f)
    common = ["--mesh_dir", str(tmp_path / "mesh"), "--root_dir", str(tmp_path), "--scans", "1", "2", "3", "--num_views", "4",
              "--img_wh", "64", "48", "--original_img_wh", "64", "48", "--offset_dist", "0.25"]
    RT.main(common + ["--out_dir", str(tmp_path / "png"), "--format", "png", "--dump_poses", str(tmp_path / "poses")])
    RT.main(common + ["--out_dir", str(tmp_path / "jpg")])
    K0, w2cs = RT.key_poses(str(tmp_path), [23, 24, 23], 0.25)
    c2ws = RT.interpolate_trajectory(w2cs, 4)
    assert not os.path.exists(tmp_path / "png" / "scan3")                     # no mesh: skipped
    for scan in meshes:
        v, f = dtu_eval.read_ply(str(tmp_path / "mesh" / f"scan{scan}.ply"))
        want = RT.render_mesh(v, f, RT.scaled_intrinsics(K0, [64, 48], [64, 48]), c2ws, 48, 64)
        assert (want != 255).any()
        for i in range(4):
            png = np.array(Image.open(tmp_path / "png" / f"scan{scan}" / f"render_{i}.png"))
            assert png.shape == (48, 64, 3) and np.array_equal(png, want[i])
            jpg = np.array(Image.open(tmp_path / "jpg" / f"scan{scan}" / f"render_{i}.jpg"))
            assert jpg.shape == (48, 64, 3) and np.abs(jpg.astype(np.int32) - want[i].astype(np.int32)).mean() < 8
        assert not os.path.exists(tmp_path / "png" / f"scan{scan}" / "render_4.png")
    for i in range(4):
        K, c2w, h, w = RT.load_pinhole_json(str(tmp_path / "poses" / f"tmp{i}.json"))
        assert (h, w) == (48, 64) and np.array_equal(K, K0.astype(np.float64))
        assert np.abs(c2w - c2ws[i]).max() <= 1e-12 * np.abs(c2ws[i]).max()
