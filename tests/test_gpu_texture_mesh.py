"""The mesh-texturing kernels (csrc/mesh_texture.hip and the textured branch of csrc/raster.hip's shade kernel) against the
numpy restatement (texture_ref.py) on the device: texture, views_used, fill states and round counts bit for bit -- both sides
form the same float64 expressions without contraction, and the depth maps the restatement is given are the device's own.
Then the textured frames against the restatement's shade, the known answers of test_texture_ref.py on the device, guard bands
round every allocation of uforecon_amd/texture_ops.py, the argument errors and the command.

tests/test_guarded_alloc.py lists the entry points of include/ufr.h that take a ``workspace_bytes`` count against the refusal
cases of tests/test_gpu_guard_bands.py.  The two texture entry points that take a workspace name their count
``workspace_size`` and have their refusal cases here (``test_short_workspace_is_refused_before_anything_is_written``), with
the same ``ShortWorkspace`` and the same snapshot of every guarded buffer."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import color_mesh_ref as CR
import texture_ref as TR
from guarded_alloc import GuardedTorch
from test_color_mesh_ref import cameras_of
from test_gpu_guard_bands import ShortWorkspace
from test_texture_ref import (FILL, check_occlusion_and_fallback, check_round_trip, check_silhouette_fill,
                              check_texture_beats_vertex_colours)
from uforecon_amd import _lib, clean_mesh as CM, dtu_eval, ops, render_trajectory as RT, texture_mesh as TM, texture_ops as TO
from uforecon_amd._lib import UfrError

pytestmark = pytest.mark.gpu

H, W, FOCAL, DIST = 48, 64, 80.0, 4.0
BLOCK = TO.TEXTURE_BLOCK                 # the texels one block of the bake and of the fill round owns: 256


def cuda(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def gpu_depth(v, f, K, c2ws, h, w):
    """(n,h,w) float32: the mesh's z-depth from every camera, one call per view as texture_mesh makes them"""
    tv, tf = cuda(np.asarray(v, np.float64)), cuda(np.asarray(f, np.int32))
    out = []
    for c2w in c2ws:
        k_inv, c32 = CM.ray_camera(K.astype(np.float32), np.linalg.inv(c2w).astype(np.float32))
        out.append(ops.raster_frames(tv, tf, k_inv, c32[None], h, w, return_depth=True, check_indices=False)["depth"][0].cpu().numpy())
    return np.stack(out)


def gpu_bake(v, f, imgs, depth, k, w, c, S, fallback=None, **kw):
    tex, used = TO.mesh_texture_bake(cuda(np.asarray(v, np.float64)), cuda(np.asarray(f, np.int32)), cuda(imgs),
                                     None if depth is None else cuda(depth), k, w, c, S,
                                     fallback=None if fallback is None else cuda(fallback), **kw)
    return tex.cpu().numpy(), used.cpu().numpy()


def gpu_fill(tex, used, F, S, rounds):
    t, st, run = TO.mesh_texture_fill(cuda(tex), cuda(used), S, F, rounds)
    return t.cpu().numpy(), st.cpu().numpy(), run


_scenes = {}


def sphere_scene(level, n_views, F=None):
    """the first ``F`` faces of an icosphere (80 faces at level 1, 320 at level 2) with all its vertices, ``n_views`` ring
    cameras, noise pictures, random fallback colours and the device's depth maps of those faces; built once per key and
    shared (never modified)"""
    key = (level, n_views, F)
    if key not in _scenes:
        v, f = CR.icosphere(level)
        f = f if F is None else f[:F]
        K = CR.intrinsics(H, W, FOCAL)
        c2ws = CR.ring_cameras(n_views, DIST, height=0.7)
        rng = np.random.default_rng(1000 * level + n_views)
        imgs = rng.integers(0, 256, (n_views, H, W, 3)).astype(np.uint8)
        k, w, c = cameras_of(K, c2ws)
        _scenes[key] = dict(v=v, f=f, K=K, c2ws=c2ws, imgs=imgs, depth=gpu_depth(v, f, K, c2ws, H, W), k=k, w=w, c=c,
                            fallback=rng.integers(0, 256, (len(v), 3)).astype(np.uint8))
    return _scenes[key]


def assert_bits(s, S, occlusion=True, fallback=True, **kw):
    kw = dict(dict(depth_tol=0.02, fill=FILL), **kw)
    depth = s["depth"] if occlusion else None
    fb = s["fallback"] if fallback else None
    got = gpu_bake(s["v"], s["f"], s["imgs"], depth, s["k"], s["w"], s["c"], S, fallback=fb, **kw)
    want = TR.bake(s["v"], s["f"], s["imgs"], depth, s["k"], s["w"], s["c"], S, fallback=fb, **kw)
    print(f"F {len(s['f'])}, S {S}: atlas {want[1].shape[1]}x{want[1].shape[0]}, seen {(want[1] > 0).sum()}, views_used histogram "
          f"{np.bincount(want[1].reshape(-1)).tolist()}, colour mismatches {(got[0] != want[0]).any(-1).sum()}, views_used mismatches "
          f"{(got[1] != want[1]).sum()}")
    assert got[0].shape == want[0].shape == TO.atlas_layout(len(s["f"]), S)[:2] + (3,)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    return got


# ------------------------------------------------------------------ the bake, bit for bit
@pytest.mark.parametrize("mode", ["mean", "best"])
@pytest.mark.parametrize("occlusion", [True, False])
def test_three_views_match_the_restatement_and_repeat(mode, occlusion):
    s = sphere_scene(1, 3)
    got = assert_bits(s, 2, mode=mode, occlusion=occlusion)
    face = TR.owner_map(80, 2)[0]
    seen = got[1][face >= 0] > 0
    assert 0.2 < seen.mean() < 1.0                                         # some texels unseen, not all
    if not occlusion:
        assert (got[1] == 1).any() and (got[1] == 2).any()                 # one view alone, and blends
    else:
        free = gpu_bake(s["v"], s["f"], s["imgs"], None, s["k"], s["w"], s["c"], 2, fallback=s["fallback"], depth_tol=0.02, fill=FILL,
                        mode=mode)
        assert (free[1] >= got[1]).all() and (free[1] > got[1]).any()      # the depth maps do hide the far side
    again = gpu_bake(s["v"], s["f"], s["imgs"], s["depth"] if occlusion else None, s["k"], s["w"], s["c"], 2, fallback=s["fallback"],
                     depth_tol=0.02, fill=FILL, mode=mode)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


@pytest.mark.parametrize("n_views,F", [(1, None), (64, 8)])
def test_one_view_and_the_most_views(n_views, F):
    assert n_views in (1, ops.MESH_MAX_VIEWS)
    got = assert_bits(sphere_scene(1, n_views, F), 2, occlusion=n_views == 1, min_cos=0.0)
    assert got[1].max() <= n_views and (got[1] > 0).any()
    if n_views == 64:
        assert got[1].max() > 16                                           # the sums do run past one upload launch's cameras


@pytest.mark.parametrize("S", [1, 2, 7])
@pytest.mark.parametrize("F", [1, 2, 3, 80])
def test_patch_sizes_and_face_counts(S, F):
    """F = 1 and 3: the last cell is half empty; F = 3 and 80: the last row of cells is partly empty (80: 40 cells in 7 x 6).
    Texels: 16 (F 1, S 1) and 100 (F 1, S 7) lie on both sides of a wave, 200 (F 3, S 7) and 672 (F 80, S 1) of a block."""
    Ht, Wt, cols, rows = TO.atlas_layout(F, S)
    if (F, S) in ((1, 1), (1, 7), (3, 7), (80, 1)):
        assert Ht * Wt == {(1, 1): 16, (1, 7): 100, (3, 7): 200, (80, 1): 672}[(F, S)] and 16 < 64 < 100 < 200 < BLOCK < 672
    if F == 80:
        assert cols * rows > (F + 1) // 2
    got = assert_bits(sphere_scene(1, 3, None if F == 80 else F), S, occlusion=F == 80, min_cos=0.0)
    face = TR.owner_map(F, S)[0]
    assert (got[1][face < 0] == 0).all() and (got[0][face < 0] == FILL).all() and (got[1][face >= 0] > 0).any()


def test_320_faces_over_many_blocks():
    s = sphere_scene(2, 3)
    assert len(s["f"]) == 320 and np.prod(TO.atlas_layout(320, 1)[:2]) > 10 * BLOCK
    assert_bits(s, 1)


@pytest.mark.parametrize("power", [0, 8])
@pytest.mark.parametrize("fallback", [True, False])
def test_weight_powers_with_and_without_fallback(power, fallback):
    assert power in (0, ops.MESH_COLOR_MAX_POWER)
    got = assert_bits(sphere_scene(1, 3), 2, occlusion=False, fallback=fallback, power=power)
    face = TR.owner_map(80, 2)[0]
    unseen = (got[1] == 0) & (face >= 0)
    assert unseen.any() and ((got[0][unseen] == FILL).all(-1).all() == (not fallback))


def test_zero_area_face_non_finite_vertex_and_index_out_of_range():
    s = sphere_scene(1, 3)
    v, f = s["v"].copy(), s["f"][:12].copy()
    f[0] = (f[0, 0], f[0, 0], f[0, 1])                                     # zero area: the zero normal, which no view sees
    f[3] = (f[3, 0], f[3, 1], len(v) + 5)                                  # out of range: fill
    f[5] = (f[5, 0], -1, f[5, 2])
    v[f[8, 1]] = (np.nan, 0.0, np.inf)                                     # its faces' texels are unseen wherever its weight counts
    depth = gpu_depth(np.nan_to_num(v, nan=0.0, posinf=0.0), f[[1, 2, 4, 6, 7]], s["K"], s["c2ws"], H, W)
    t = dict(s, v=v, f=f, depth=depth)
    for fallback in (True, False):
        got = assert_bits(t, 2, fallback=fallback, min_cos=0.0)
        face = TR.owner_map(12, 2)[0]
        for dead in (3, 5):
            assert (got[1][face == dead] == 0).all() and (got[0][face == dead] == FILL).all()
        assert (got[1][face == 0] == 0).all() and (got[1][face == 8] == 0).all() and (got[1] > 0).any()


# ------------------------------------------------------------------ the fill
@pytest.mark.parametrize("rounds", [0, 1, 2, 1000])
def test_fill_matches_the_restatement(rounds):
    s = sphere_scene(1, 3)
    S, F = 2, 80
    tex, used = gpu_bake(s["v"], s["f"], s["imgs"], s["depth"], s["k"], s["w"], s["c"], S, fallback=s["fallback"], depth_tol=0.02, fill=FILL)
    want = TR.fill(tex, used, F, S, rounds)
    t, st, run = gpu_fill(tex, used, F, S, rounds)
    print(f"rounds {rounds}: run {run}, coloured {(st != 0).sum()} of {st.size}")
    assert run == want[2] and np.array_equal(st, want[1]) and np.array_equal(t, want[0])
    if rounds == 0:
        assert run == 0 and np.array_equal(t, tex) and np.array_equal(st != 0, used != 0)
    if rounds == 1000:
        assert 2 < run < 12                                                # stopped early: a patch of S = 2 is five texels across
        again = gpu_fill(tex, used, F, S, rounds)
        assert again[2] == run and np.array_equal(again[0], t) and np.array_equal(again[1], st)


# ------------------------------------------------------------------ textured frames
def frames_scene():
    if "frames" not in _scenes:
        s = sphere_scene(1, 3)
        S = 2
        Ht, Wt, _, _ = TO.atlas_layout(80, S)
        rng = np.random.default_rng(77)
        texture = rng.integers(0, 256, (Ht, Wt, 3)).astype(np.uint8)
        k_inv = CM.ray_camera(s["K"].astype(np.float32), np.eye(4, dtype=np.float32))[0]
        c2ws = s["c2ws"][:2].astype(np.float32)
        hits = [TR.RR.first_hit(s["v"], s["f"], k_inv, c, np.ones((H, W), bool), return_close=True) for c in c2ws]
        # texel coordinates on the atlas border and past it: both clamps, at both ends of both axes
        wild = rng.uniform(-1.5, 1.5, (80, 3, 2)) + rng.integers(0, 2, (80, 3, 2)) * np.array([Wt - 1.0, Ht - 1.0])
        wild[:20] = np.round(wild[:20])                                    # and exactly on texel centres, the border's included
        _scenes["frames"] = dict(s, S=S, texture=texture, k_inv=k_inv, c2ws32=c2ws, hits=hits, normals=TR.RR.vertex_normals(s["v"], s["f"]),
                                 xy=dict(atlas=TO.corner_texels(80, S), wild=wild))
    return _scenes["frames"]


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("coords", ["atlas", "wild"])
def test_textured_frames_match_the_restatement(smooth, coords):
    s = frames_scene()
    tv, tf = cuda(s["v"]), cuda(s["f"])
    tn = ops.raster_vertex_normals(tv, tf) if smooth else None
    xy = s["xy"][coords]
    got = TO.raster_frames_textured(tv, tf, s["k_inv"], s["c2ws32"], H, W, cuda(xy), cuda(s["texture"]), normals=tn, ambient=0.3,
                                    return_depth=True, return_face_ids=True, return_normals=True)
    plain = ops.raster_frames(tv, tf, s["k_inv"], s["c2ws32"], H, W, normals=tn, colors=cuda(s["fallback"]), ambient=0.3,
                              return_depth=True, return_face_ids=True, return_normals=True)
    for key in ("depth", "face_id", "normal"):                             # the outputs the two entry points share: the same bits
        assert np.array_equal(got[key].cpu().numpy(), plain[key].cpu().numpy()), key
    for i in range(2):
        want = TR.render(s["v"], s["f"], s["k_inv"], s["c2ws32"][i], H, W, xy, s["texture"], normals=s["normals"] if smooth else None,
                         ambient=0.3, hit=s["hits"][i])
        image = got["image"][i].cpu().numpy()
        close = want["close"]
        diff = np.abs(image.astype(np.int32) - want["image"].astype(np.int32)).max(-1)
        print(f"frame {i}: close share {close.mean():.4f}, image diff max {diff.max()}, hit pixels {(want['face_id'] >= 0).sum()}")
        assert close.mean() <= 0.005 and (diff[~close] == 0).all() and (diff <= 1).all()
        assert np.array_equal(got["face_id"][i].cpu().numpy()[~close], want["face_id"][~close])
        ulp = np.spacing(np.abs(want["depth"]).astype(np.float32))
        assert (np.abs(got["depth"][i].cpu().numpy().astype(np.float64) - want["depth"].astype(np.float64)) <= ulp).all()
        assert (want["face_id"] >= 0).sum() > 300 and len(np.unique(image.reshape(-1, 3), axis=0)) > 100


def test_vertex_colour_frames_are_what_they_were_beside_the_textured_ones():
    """``ops.raster_frames`` with vertex colours before and after a textured call on the same mesh: the same bits, and its depth
    and face ids are the textured call's"""
    s = frames_scene()
    tv, tf, tc = cuda(s["v"]), cuda(s["f"]), cuda(s["fallback"])
    want = TR.RR.render(s["v"], s["f"], s["k_inv"], s["c2ws32"][0], H, W, colors=s["fallback"], hit=s["hits"][0])
    kw = dict(colors=tc, return_depth=True, return_face_ids=True)
    before = ops.raster_frames(tv, tf, s["k_inv"], s["c2ws32"][:1], H, W, **kw)
    tex = TO.raster_frames_textured(tv, tf, s["k_inv"], s["c2ws32"][:1], H, W, cuda(s["xy"]["atlas"]), cuda(s["texture"]),
                                    return_depth=True, return_face_ids=True)
    after = ops.raster_frames(tv, tf, s["k_inv"], s["c2ws32"][:1], H, W, **kw)
    for key in ("image", "depth", "face_id"):
        assert np.array_equal(before[key].cpu().numpy(), after[key].cpu().numpy()), key
    assert np.array_equal(tex["depth"].cpu().numpy(), before["depth"].cpu().numpy())
    assert np.array_equal(tex["face_id"].cpu().numpy(), before["face_id"].cpu().numpy())
    ok = ~want["close"]
    assert np.array_equal(before["image"][0].cpu().numpy()[ok], want["image"][ok])


def test_a_texture_coordinate_that_is_not_finite_gives_white():
    s = frames_scene()
    xy = s["xy"]["atlas"].copy()
    xy[:, 0, 0] = np.nan
    got = TO.raster_frames_textured(cuda(s["v"]), cuda(s["f"]), s["k_inv"], s["c2ws32"][:1], H, W, cuda(xy), cuda(s["texture"]),
                                    ambient=1.0, background=(0, 0, 0), return_face_ids=True)
    hit = got["face_id"][0].cpu().numpy() >= 0
    image = got["image"][0].cpu().numpy()
    assert hit.sum() > 300 and (image[hit] == 255).all() and (image[~hit] == 0).all()


# ------------------------------------------------------------------ known answers on the device
class DeviceSide:
    """the operations of test_texture_ref.py's known answers, on the device"""

    def bake(self, s, S, depth=None, fallback=None, **kw):
        k, w, c = s["cams"]
        return gpu_bake(s["v"], s["f"], s["imgs"], depth, k, w, c, S, fallback=fallback, **kw)

    def depth(self, s):
        return gpu_depth(s["v"], s["f"], s["K"], s["c2ws"], s["H"], s["W"])

    def fill(self, tex, used, F, S, rounds):
        return gpu_fill(tex, used, F, S, rounds)

    def render(self, s, xy, tex, ambient=1.0):
        r = TO.raster_frames_textured(cuda(s["v"]), cuda(s["f"]), s["k_inv"], s["c2ws"][:1].astype(np.float32), s["H"], s["W"], cuda(xy),
                                      cuda(tex), ambient=ambient, return_face_ids=True)
        return r["image"][0].cpu().numpy(), r["face_id"][0].cpu().numpy()

    def vertex_render(self, s, ambient=1.0):
        k, w, c = s["cams"]
        tv, tf = cuda(s["v"]), cuda(s["f"])
        colors, _ = ops.mesh_vertex_colors(tv, ops.raster_vertex_normals(tv, tf), cuda(s["imgs"]), None, k, w, c, min_cos=0.0, fill=FILL)
        return ops.raster_frames(tv, tf, s["k_inv"], s["c2ws"][:1].astype(np.float32), s["H"], s["W"], colors=colors,
                                 ambient=ambient)["image"][0].cpu().numpy()


def test_round_trip_on_the_device():
    check_round_trip(DeviceSide())


def test_silhouette_fill_on_the_device():
    check_silhouette_fill(DeviceSide())


def test_occlusion_and_fallback_on_the_device():
    check_occlusion_and_fallback(DeviceSide())


def test_texture_beats_vertex_colours_on_the_device():
    check_texture_beats_vertex_colours(DeviceSide())


# ------------------------------------------------------------------ guard bands
def _guarded_run(put):
    """bake, fill and textured frames of the 80-face sphere, every input placed between guards by ``put``"""
    s = frames_scene()
    tv, tf = put(cuda(s["v"])), put(cuda(s["f"]))
    tex, used = TO.mesh_texture_bake(tv, tf, put(cuda(s["imgs"])), put(cuda(s["depth"])), s["k"], s["w"], s["c"], s["S"],
                                     fallback=put(cuda(s["fallback"])), depth_tol=0.02, fill=FILL)
    filled, state, runs = TO.mesh_texture_fill(tex, used, s["S"], 80, 2)
    frames = TO.raster_frames_textured(tv, tf, s["k_inv"], s["c2ws32"], H, W, put(cuda(s["xy"]["wild"])), filled,
                                       normals=put(ops.raster_vertex_normals(tv, tf)), return_depth=True, return_face_ids=True,
                                       return_normals=True)
    return dict(tex=tex, used=used, filled=filled, state=state, runs=runs, **frames)


def test_guard_bands_round_every_allocation(monkeypatch):
    """texture_ops allocates no floating ``empty`` output (depth and normal maps are ``zeros``, the rest is uint8 or int32), so
    "written in full" is checked the other way: every guarded output equals the unguarded run's, which the tests above tie to
    the restatement"""
    want = _guarded_run(lambda t: t)
    g = GuardedTorch().install(monkeypatch, TO)
    got = _guarded_run(g.place)
    g.check()
    assert g.guarded >= 10 and g.placed == 7
    assert got["runs"] == want["runs"] == 2
    for key in ("tex", "used", "filled", "state", "image", "depth", "face_id", "normal"):
        assert np.array_equal(got[key].cpu().numpy(), want[key].cpu().numpy()), key
    assert (got["face_id"].cpu().numpy() >= 0).sum() > 600 and (got["used"].cpu().numpy() > 0).any()


@pytest.mark.parametrize("entry", ["ufr_texture_bake", "ufr_texture_frames"])
def test_short_workspace_is_refused_before_anything_is_written(entry, monkeypatch):
    index = _lib.SIGNATURES[entry][1].index(_lib.sz)                       # the one size_t: workspace_size
    guard = GuardedTorch().install(monkeypatch, TO)
    lib = ShortWorkspace(_lib.load(), entry, index, guard)
    monkeypatch.setattr(_lib, "_lib", lib)
    with pytest.raises(UfrError) as e:
        _guarded_run(guard.place)
    assert lib.asked is not None and lib.asked > 0, f"{entry}: the run never called it"
    assert lib.rc == -1 and "(-1)" in str(e.value)                         # UFR_ERR_ARG, as ufr_color_vertices and ufr_raster_frames
    assert f": workspace too small: {lib.asked - 1} < {lib.asked} bytes" in str(e.value), str(e.value)
    guard.check()
    changed = guard.changed(lib.before)
    assert not changed, f"{entry}: refused, yet {len(changed)} buffer(s) were written:\n  " + "\n  ".join(changed)


# ------------------------------------------------------------------ argument errors
def test_argument_errors_raise_with_the_reason_and_launch_nothing():
    import torch

    s = frames_scene()
    tv, tf, imgs = cuda(s["v"]), cuda(s["f"]), cuda(s["imgs"])
    k, w, c = s["k"], s["w"], s["c"]
    Ht, Wt, _, _ = TO.atlas_layout(80, 2)

    def bad(reason, **kw):
        a = dict(verts=tv, faces=tf, images=imgs, depth=None, k=k, w2c=w, centre=c, S=2)
        a.update(kw)
        with pytest.raises(UfrError) as e:
            TO.mesh_texture_bake(**a)
        assert reason in str(e.value), (reason, str(e.value))

    ops.profile_enable(True)                       # every launch of the library is recorded from here on
    bad("S 0", S=0)
    bad("S 126", S=126)
    bad("16384", faces=torch.zeros((2 * 130 * 130, 3), dtype=torch.int32, device="cuda"), S=125)
    bad("views", images=imgs[:0], k=k[:0], w2c=w[:0], centre=c[:0])
    bad("image", images=imgs[:, :1].contiguous())
    bad("dtype", images=imgs.float())
    bad("depth", depth=torch.zeros((3, H, W + 1), dtype=torch.float32, device="cuda"))
    bad("fallback", fallback=torch.zeros((5, 3), dtype=torch.uint8, device="cuda"))
    bad("faces", faces=torch.zeros((80, 4), dtype=torch.int32, device="cuda"))
    bad("power", power=9)
    bad("mode", mode="median")
    bad("min_cos", min_cos=1.5)
    bad("depth_tol", depth_tol=-1.0)
    bad("z_min", z_min=float("inf"))
    ws = w.copy()
    ws[1, 2, :3] = 0.0
    bad("singular", w2c=ws)
    tex, used = torch.zeros((Ht, Wt, 3), dtype=torch.uint8, device="cuda"), torch.zeros((Ht, Wt), dtype=torch.uint8, device="cuda")
    for reason, call in (("closed form", lambda: TO.mesh_texture_fill(tex, used, 2, 60, 1)),
                         ("closed form", lambda: TO.mesh_texture_fill(tex, used, 3, 80, 1)),
                         ("rounds", lambda: TO.mesh_texture_fill(tex, used, 2, 80, -1)),
                         ("expected", lambda: TO.mesh_texture_fill(tex, used[:-1], 2, 80, 1)),
                         ("corner_xy", lambda: TO.raster_frames_textured(tv, tf, s["k_inv"], s["c2ws32"], H, W, cuda(s["xy"]["atlas"][:-1]), tex)),
                         ("texture", lambda: TO.raster_frames_textured(tv, tf, s["k_inv"], s["c2ws32"], H, W, cuda(s["xy"]["atlas"]), used)),
                         ("ambient", lambda: TO.raster_frames_textured(tv, tf, s["k_inv"], s["c2ws32"], H, W, cuda(s["xy"]["atlas"]), tex,
                                                                        ambient=1.5))):
        with pytest.raises(UfrError) as e:
            call()
        assert reason in str(e.value), (reason, str(e.value))
    # the library itself refuses what the wrappers refuse: straight through ctypes
    lib = _lib.load()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    fill = (C.c_uint8 * 3)(1, 2, 3)
    p = tv.data_ptr()
    kd, wd, cd = (np.ascontiguousarray(a).ctypes.data_as(dp) for a in (k, w, c))

    def bake(F=80, S=2, ht=Ht, wt=Wt, n=3, h=H, wd_=W, power=2, mode=0, min_cos=0.2, verts=p, texture=p, ww=wd, ws_bytes=1 << 16):
        return lib.ufr_texture_bake(verts, p, 100, F, p, None, kd, ww, cd, n, h, wd_, S, ht, wt, 0.0, 0.005, min_cos, power, mode, fill,
                                    None, texture, p, p, ws_bytes, None)

    for reason, kw in ((b"null", dict(verts=None)), (b"null", dict(texture=None)), (b"S 0", dict(S=0)), (b"S 126", dict(S=126)),
                       (b"closed form", dict(ht=Ht + 1)), (b"closed form", dict(wt=Wt - 1)), (b"closed form", dict(F=79, ht=Ht - 4)),
                       (b"atlas", dict(ht=16385)), (b"atlas", dict(wt=0)), (b"side above", dict(F=2 * 130 * 130, S=125)),
                       (b"n_views", dict(n=0)), (b"n_views", dict(n=65)), (b"image", dict(h=1)), (b"power", dict(power=9)),
                       (b"mode", dict(mode=2)), (b"min_cos", dict(min_cos=1.5)), (b"singular", dict(ww=np.ascontiguousarray(ws).ctypes.data_as(dp))),
                       (b"workspace too small", dict(ws_bytes=8))):
        assert bake(**kw) == -1 and reason in lib.ufr_last_error(), (kw, lib.ufr_last_error())
    assert lib.ufr_texture_fill_round(None, p, 2, Ht, Wt, 80, p, p, p, None) == -1 and b"null" in lib.ufr_last_error()
    assert lib.ufr_texture_fill_round(p, p, 2, Ht, Wt, 80, p, p, p, None) == -1 and b"alias" in lib.ufr_last_error()
    assert lib.ufr_texture_fill_round(p, p, 2, Ht, Wt + 5, 80, tex.data_ptr(), used.data_ptr(), p, None) == -1 and b"closed form" in lib.ufr_last_error()
    kinv = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    c2w = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)

    def frames(xy=p, texture=p, ht=4, wt=4, h=4, wd_=4, ambient=0.25, ws_bytes=1 << 16):
        return lib.ufr_texture_frames(p, p, 1, 1, None, xy, texture, ht, wt, C.cast(kinv, fp), C.cast(c2w, fp), 1, h, wd_, None, ambient, p,
                                      None, None, None, p, ws_bytes, None)

    for reason, kw in ((b"null", dict(xy=None)), (b"null", dict(texture=None)), (b"texture", dict(ht=0)), (b"texture", dict(wt=16385)),
                       (b"image", dict(h=0)), (b"ambient", dict(ambient=1.5)), (b"workspace too small", dict(ws_bytes=64))):
        assert frames(**kw) == -1 and reason in lib.ufr_last_error(), (kw, lib.ufr_last_error())
    launched = ops.profile_read()
    ops.profile_enable(False)
    assert launched == {}, launched
    with pytest.raises(UfrError):
        RT.render_mesh(s["v"], s["f"], s["K"], s["c2ws"][:1], H, W, texture=s["texture"])                     # without corner_xy
    with pytest.raises(UfrError):
        TM.texture_mesh(s["v"], s["f"], [], [])
    with pytest.raises(UfrError):
        TM.texture_mesh(s["v"], s["f"] + 40, [(s["K"], np.eye(4))], [s["imgs"][0]])


# ------------------------------------------------------------------ the command
def test_command_end_to_end(tmp_path, capsys):
    from PIL import Image

    root, mesh_dir, out_dir, frames_dir = (str(tmp_path / d) for d in ("dtu", "mesh", "texture", "frames"))
    os.makedirs(mesh_dir)
    views, scans = [3, 11, 24], [7, 9]
    K = CR.intrinsics(H, W, FOCAL)
    c2ws = CR.ring_cameras(3, DIST, height=0.7)
    rng = np.random.default_rng(21)
    pics = {s: [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in views] for s in scans}
    CR.write_dtu_tree(root, scans, views, K, c2ws, pics)
    meshes = {7: CR.icosphere(1), 9: CR.icosphere(1, radius=0.8, centre=(0.1, 0.0, 0.05))}
    for s, (v, f) in meshes.items():
        CM.write_ply(os.path.join(mesh_dir, "scan%d.ply" % s), v, f)
    assert TM.main(["--mesh_dir", mesh_dir, "--root_dir", root, "--out_dir", out_dir, "--scans", "7", "9", "--views", "3", "11", "24",
                    "--depth_tol", "0.02", "--patch", "3"]) == 0
    out = capsys.readouterr().out
    report = json.load(open(os.path.join(out_dir, "texture_mesh.json")))
    assert sorted(report) == ["scan7", "scan9"]
    cams = [CM.read_cam_file(os.path.join(root, "cameras/{:0>8}_cam.txt".format(i))) for i in views]
    for s in scans:
        name = "scan%d" % s
        v, f, xy, tex = TM.read_obj(os.path.join(out_dir, name + ".obj"))
        v0, f0 = dtu_eval.read_ply(os.path.join(mesh_dir, name + ".ply"))
        assert np.array_equal(v, v0) and np.array_equal(f, f0)
        want_tex, want_xy, used, state = TM.texture_mesh(v0, f0, cams, pics[s], patch=3, depth_tol=0.02)
        assert np.array_equal(tex, want_tex) and np.abs(xy - want_xy).max() < 1e-9 and np.array_equal(want_xy, TO.corner_texels(80, 3))
        r = report[name]
        assert r["faces"] == 80 and r["patch"] == 3 and r["atlas"] == [want_tex.shape[1], want_tex.shape[0]] and r["views"] == views
        counts = np.bincount(state.reshape(-1), minlength=5)
        assert r["texels"] == dict(zip(TM.STATE_NAMES, (int(n) for n in counts))) and counts.sum() == state.size
        assert counts[TM.STATE_SEEN] > 0 and counts[TM.STATE_FILLED] > 0 and counts[TM.STATE_FALLBACK] > 0 and counts[TM.STATE_EMPTY] == 0
        assert counts[TM.STATE_NO_FACE] == (TR.owner_map(80, 3)[0] < 0).sum() and np.array_equal(state == TM.STATE_SEEN, used > 0)
        assert all(k in r for k in ("upload_ms", "depth_ms", "fallback_ms", "bake_ms", "fill_ms", "fill_rounds_run"))
        assert "%s: 80 faces, S 3" % name in out
    args = ["--root_dir", root, "--scans", "7", "--views", "3", "11", "--num_views", "2", "--img_wh", "64", "48", "--original_img_wh", "64",
            "48", "--offset_dist", "0.25", "--format", "png", "--color", "texture"]
    RT.main(["--mesh_dir", out_dir, "--out_dir", frames_dir] + args)
    v, f, xy, tex = TM.read_obj(os.path.join(out_dir, "scan7.obj"))
    K0, w2cs = RT.key_poses(root, [3, 11], 0.25)
    want = RT.render_mesh(v, f, RT.scaled_intrinsics(K0, [64, 48], [64, 48]), RT.interpolate_trajectory(w2cs, 2), 48, 64, texture=tex,
                          corner_xy=xy)
    plain = RT.render_mesh(v, f, RT.scaled_intrinsics(K0, [64, 48], [64, 48]), RT.interpolate_trajectory(w2cs, 2), 48, 64)
    for i in range(2):
        png = np.array(Image.open(os.path.join(frames_dir, "scan7", "render_%d.png" % i)))
        assert png.shape == (48, 64, 3) and np.array_equal(png, want[i])
        assert len(np.unique(png.reshape(-1, 3), axis=0)) > 100 and not np.array_equal(png, plain[i])
    no_fb = TM.texture_mesh(v0, f0, cams, pics[9], patch=3, depth_tol=0.02, vertex_fallback=False, fill_rounds=0)
    assert ((no_fb[3] == TM.STATE_EMPTY) == ((no_fb[2] == 0) & (no_fb[3] != TM.STATE_NO_FACE))).all() and (no_fb[3] == TM.STATE_EMPTY).any()
    assert (no_fb[0][no_fb[3] == TM.STATE_EMPTY] == np.array(TM.FILL_COLOR, np.uint8)).all()
