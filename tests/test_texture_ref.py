"""Mesh texturing without a GPU: the closed-form atlas (tests/texture_ref.py against uforecon_amd/texture_ops.py), the known
answers of the numpy statement, the fill-round rule, the header and the binding, the OBJ / MTL / PNG files and the command's
failure lines.  The scenes and their checks are shared with tests/test_gpu_texture_mesh.py, which runs them on the device."""
import inspect
import json
import os
import re

import numpy as np
import pytest

import color_mesh_ref as CR
import raster_ref as RR
import texture_ref as TR
from test_color_mesh_ref import cameras_of, grid_square, ref_depth
from uforecon_amd import clean_mesh as CM, color_mesh as CMesh, render_trajectory as RT, texture_mesh as TM, texture_ops as TO
from uforecon_amd._lib import UfrError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILL = (7, 8, 9)
LAYOUT_S = range(1, 9)
LAYOUT_F = (1, 2, 3, 7, 80)


# ------------------------------------------------------------------ the atlas
@pytest.mark.parametrize("F", LAYOUT_F)
def test_every_texel_has_one_owner_or_none_and_the_corners_are_as_stated(F):
    for S in LAYOUT_S:
        Ht, Wt, cols, rows = TR.layout(F, S)
        C = S + 3
        cells = (F + 1) // 2
        assert (Ht, Wt, cols, rows) == TO.atlas_layout(F, S) and Ht == rows * C and Wt == cols * C
        assert (cols - 1) ** 2 < cells <= cols * cols and (rows - 1) * cols < cells <= rows * cols
        face, li, lj = TR.owner_map(F, S)
        assert face.min() >= -1 and face.max() == F - 1
        assert np.array_equal(TM.texel_has_face(F, S), face >= 0)
        for f in range(F):                                        # a face owns the texels of one cell only, and how many
            ys, xs = np.nonzero(face == f)
            q = f // 2
            assert (xs // C == q % cols).all() and (ys // C == q // cols).all()
            # even: i + j <= S + 2 inside a C x C cell; odd: what is left, i' + j' <= S + 1
            assert len(xs) == ((S + 3) * (S + 4) // 2 if f % 2 == 0 else (S + 2) * (S + 3) // 2)
            assert (li[ys, xs] + lj[ys, xs] <= S + 2 - (f % 2)).all() and li[ys, xs].min() == 0 == lj[ys, xs].min()
        if F % 2:                                                 # the last cell is half empty
            assert (face == -1).sum() >= (S + 2) * (S + 3) // 2
        xy = TR.corner_texels(F, S)
        assert np.array_equal(xy, TO.corner_texels(F, S)) and xy.dtype == np.float64
        for f in range(F):
            got = [TR.owner(F, S, int(x), int(y)) for x, y in xy[f]]
            assert got == [(f, 0, 0), (f, S, 0), (f, 0, S)]
            ox, oy = (f // 2 % cols) * C, (f // 2 // cols) * C
            want = [(0, 0), (S, 0), (0, S)] if f % 2 == 0 else [(C - 1, C - 1), (C - 1 - S, C - 1), (C - 1, C - 1 - S)]
            assert [(int(x) - ox, int(y) - oy) for x, y in xy[f]] == want
            (xa, ya), (xb, yb), (xc, yc) = xy[f]                   # a half turn keeps the orientation: nothing is mirrored
            assert ((xb - xa) * (yc - ya) - (yb - ya) * (xc - xa) > 0)


@pytest.mark.parametrize("F", LAYOUT_F)
def test_the_bilinear_footprint_of_a_face_stays_on_its_own_texels(F):
    """Barycentrics in 64ths: with corner coordinates below 2^11 every product and sum below is exact, so a point on an edge
    lies on it exactly, as the shade kernel's own barycentrics put a point of an edge on it up to their rounding."""
    rng = np.random.default_rng(F)
    for S in LAYOUT_S:
        xy = TR.corner_texels(F, S)
        Ht, Wt, _, _ = TR.layout(F, S)
        pts = [(64, 0), (0, 64), (0, 0), (32, 32), (64 - 1, 1), (1, 64 - 1), (17, 0), (0, 45), (45, 19), (13, 51)]     # corners, edges
        pts += [(int(p), int(rng.integers(0, 65 - p))) for p in rng.integers(0, 65, 30)]                               # anywhere
        for f in sorted({0, 1 % F, F // 2, F - 1}):
            for pb, pc in pts:
                wb, wc = pb / 64.0, pc / 64.0
                wa = (1.0 - wb) - wc
                tx = (wa * xy[f, 0, 0] + wb * xy[f, 1, 0]) + wc * xy[f, 2, 0]
                ty = (wa * xy[f, 0, 1] + wb * xy[f, 1, 1]) + wc * xy[f, 2, 1]
                total = 0.0
                for x, y, w in TR.footprint(tx, ty):
                    if w != 0.0:
                        assert 0 <= x < Wt and 0 <= y < Ht and TR.owner(F, S, x, y)[0] == f, (F, S, f, pb, pc, x, y, w)
                    total += w
                assert abs(total - 1.0) < 1e-12


def test_patch_for_atlas_is_maximal_and_raises_when_nothing_fits():
    for F in LAYOUT_F + (3861, 400000):
        for size in (4, 5, 64, 100, 1000, 4096, 16384):
            cells = (F + 1) // 2
            cols = TR.layout(F, 1)[2]
            if cols * 4 > size:
                with pytest.raises(UfrError):
                    TO.patch_for_atlas(F, size)
                continue
            S = TO.patch_for_atlas(F, size)
            Ht, Wt, _, _ = TO.atlas_layout(F, S)
            assert 1 <= S <= 125 and Ht <= size and Wt <= size and cells <= (Wt // (S + 3)) * (Ht // (S + 3))
            if S < 125:
                assert cols * (S + 1 + 3) > size                  # the next patch size is too wide
    assert TO.patch_for_atlas(2, 4096) == 125 and TO.patch_for_atlas(80, 70) == 7 and TO.patch_for_atlas(80, 69) == 6
    for bad in (lambda: TO.atlas_layout(2, 0), lambda: TO.atlas_layout(2, 126), lambda: TO.atlas_layout(0, 4),
                lambda: TO.atlas_layout(2 * 200 * 200, 125), lambda: TO.patch_for_atlas(80, 0)):
        with pytest.raises(UfrError):
            bad()


# ------------------------------------------------------------------ the scenes the CPU and the GPU tests share
class NumpySide:
    """the three operations of a known answer, by the numpy statement"""

    def bake(self, s, S, depth=None, fallback=None, **kw):
        k, w, c = s["cams"]
        return TR.bake(s["v"], s["f"], s["imgs"], depth, k, w, c, S, fallback=fallback, **kw)

    def depth(self, s):
        return np.stack([ref_depth(s["v"], s["f"], s["K"], c, s["H"], s["W"]) for c in s["c2ws"]])

    def fill(self, tex, used, F, S, rounds):
        return TR.fill(tex, used, F, S, rounds)

    def render(self, s, xy, tex, ambient=1.0):
        r = TR.render(s["v"], s["f"], s["k_inv"], s["c2ws"][0].astype(np.float32), s["H"], s["W"], xy, tex, ambient=ambient)
        return r["image"], r["face_id"]

    def vertex_render(self, s, ambient=1.0):
        k, w, c = s["cams"]
        n = RR.vertex_normals(s["v"], s["f"])
        colors, _ = CR.vertex_colors(s["v"], n, s["imgs"], None, k, w, c, min_cos=0.0, fill=FILL)
        return RR.render(s["v"], s["f"], s["k_inv"], s["c2ws"][0].astype(np.float32), s["H"], s["W"], colors=colors, ambient=ambient)["image"]


def _scene(v, f, K, c2ws, imgs):
    H, W = imgs.shape[1:3]
    return dict(v=np.asarray(v, np.float64), f=np.asarray(f, np.int32), K=K, c2ws=np.asarray(c2ws, np.float64), imgs=imgs, H=H, W=W,
                cams=cameras_of(K, c2ws), k_inv=np.linalg.inv(K / K[2, 2]).astype(np.float32))


def square_scene(focal):
    """Two triangles form the square [-1,1]^2 at z = 0; both hypotenuses are outer edges, so both gutters leave the square.  The
    camera stands at (0.3, 0.2, 4) and looks at the origin; the picture is 48 x 64 with a linear ramp per channel: x + y, 2x,
    3y (slopes of 1 to 3 grey levels a pixel)."""
    H, W = 48, 64
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([xs + ys, 2 * xs, 3 * ys], -1).astype(np.uint8)
    v = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]
    return _scene(v, [(0, 1, 2), (0, 2, 3)], CR.intrinsics(H, W, focal), [CR.look_at((0.3, 0.2, 4.0), up=(0.0, 1.0, 0.0))], img[None])


def check_round_trip(side):
    """Known answer 1.  At focal 60 the square and its gutters project inside the picture: every texel is seen, and the textured
    square rendered from the same camera (ambient 1: no shading) reproduces the photograph at every pixel of the square within
    1 grey level: half a level from the texel's byte and half from the pixel's.  (The projective part of the camera's map
    bends a ramp by under 0.01 levels across a texel: the camera is 5 degrees off the square's axis.)"""
    s, S = square_scene(60.0), 8
    tex, used = side.bake(s, S, min_cos=0.0, fill=FILL)
    face = TR.owner_map(2, S)[0]
    assert (used[face >= 0] == 1).all() and (used[face < 0] == 0).all() and (tex[face < 0] == FILL).all()
    image, fid = side.render(s, TR.corner_texels(2, S), tex)
    on = fid >= 0
    err = np.abs(image[on].astype(int) - s["imgs"][0][on].astype(int))
    print("round trip: %d pixels, largest error %d" % (on.sum(), err.max()))
    assert on.sum() > 880 and err.max() <= 1
    return int(on.sum())


def check_silhouette_fill(side):
    """Known answer 2.  At focal 80 the gutter past the edge y = 1 projects below the picture: 13 texels are unseen (the ten
    of the odd face's gutter and three of the even face's, at its corner c), and two rounds fill them all.  Rendered from the same camera, the fill colour bleeds into the pixels
    along that edge without the fill (28 levels in the numpy statement) and the neighbour means do not (3 levels: a filled
    texel stands in for one a step of 2.5 pixels further out, on ramps of up to 3 levels a pixel, weighted by under a half).
    Asserted: with fill <= 3 and without fill > 3."""
    s, S = square_scene(80.0), 8
    tex, used = side.bake(s, S, min_cos=0.0, fill=(128, 128, 128))
    face = TR.owner_map(2, S)[0]
    assert ((used == 0) & (face >= 0)).sum() == 13 and ((used == 0) & (face == 1)).sum() == 10
    tex2, state, runs = side.fill(tex, used, 2, S, 2)
    assert runs == 2 and ((state == 0) & (face >= 0)).sum() == 0 and (state[face < 0] == 0).all()
    assert np.array_equal(tex2[used > 0], tex[used > 0])
    xy = TR.corner_texels(2, S)
    errs = []
    for t in (tex, tex2):
        image, fid = side.render(s, xy, t)
        on = fid >= 0
        errs.append(int(np.abs(image[on].astype(int) - s["imgs"][0][on].astype(int)).max()))
    print("silhouette: largest error without fill %d, with fill %d, over %d pixels" % (errs[0], errs[1], on.sum()))
    assert errs[1] <= 3 < errs[0]


def two_squares_scene():
    """A far square (half 1.5, z = 6) and a near one (half 0.6, z = 4) that hides the far one's middle from the one camera, at
    the origin looking along +z (focal 40: the near square covers |X|, |Y| < 0.9 of the far one, a pixel is 0.15 there)."""
    H, W = 48, 64
    far_v, far_f = grid_square(2, 1.5, 6.0)
    near_v, near_f = grid_square(2, 0.6, 4.0)
    rng = np.random.default_rng(5)
    s = _scene(np.concatenate([far_v, near_v]), np.concatenate([far_f, near_f + 4]), CR.intrinsics(H, W, 40.0), [np.eye(4)],
               rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8))
    s["fallback"] = rng.integers(0, 256, (8, 3)).astype(np.uint8)
    return s


def check_occlusion_and_fallback(side):
    """Known answer 3.  The far square's texels behind the near one are unseen: with ``fallback`` they hold the barycentric
    mix of their face's vertex colours, without it ``fill``; texels clear of the near square's outline by more than a pixel
    are seen, and the near square is seen everywhere.  The counts add up."""
    s, S = two_squares_scene(), 8
    depth = side.depth(s)
    face, li, lj = TR.owner_map(4, S)
    with_fb = side.bake(s, S, depth=depth, fallback=s["fallback"], min_cos=0.0, depth_tol=0.1, fill=FILL)
    without = side.bake(s, S, depth=depth, min_cos=0.0, depth_tol=0.1, fill=FILL)
    assert np.array_equal(with_fb[1], without[1])
    used = without[1]
    hidden = seen = 0
    for y, x in zip(*np.nonzero((face >= 0) & (face < 2))):
        f, i, j = face[y, x], li[y, x], lj[y, x]
        wa, wb, wc = TR.weights(i, j, S)
        a, b, c = (s["v"][t] for t in s["f"][f])
        p = (wa * a + wb * b) + wc * c
        if max(abs(p[0]), abs(p[1])) < 0.74:
            hidden += 1
            assert used[y, x] == 0 and tuple(without[0][y, x]) == FILL
            Ca, Cb, Cc = (s["fallback"][t].astype(np.float64) for t in s["f"][f])
            assert tuple(with_fb[0][y, x]) == tuple(CR._to_byte(float((wa * Ca[t] + wb * Cb[t]) + wc * Cc[t])) for t in range(3))
        elif 1.06 < max(abs(p[0]), abs(p[1])) < 1.34 and wa >= 0:     # and a pixel inside the far square's own outline
            seen += 1
            assert used[y, x] == 1 and np.array_equal(with_fb[0][y, x], without[0][y, x])
    assert hidden > 10 and seen > 10
    near = (face >= 2) & (li + lj <= S)
    assert (used[near] == 1).all()
    assert (used[face < 0] == 0).all() and (without[0][face < 0] == FILL).all() and (with_fb[0][face < 0] == FILL).all()
    n_seen, n_unseen, n_none = (used > 0).sum(), ((used == 0) & (face >= 0)).sum(), (face < 0).sum()
    assert n_seen + n_unseen + n_none == used.size and n_none == 0 and n_unseen >= hidden
    return with_fb, without


def checker_scene():
    """A 3 x 3-vertex square (8 faces, edges of 15 pixels at focal 60, z = 4) under a checkerboard of 4-pixel squares, seen by
    one frontal camera: the picture's period is shorter than a mesh edge"""
    H, W = 48, 64
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.where(((xs // 4 + ys // 4) % 2 == 0)[..., None], np.array([230, 220, 40]), np.array([20, 60, 200])).astype(np.uint8)
    v, f = grid_square(3, 1.0, 4.0)
    return _scene(v, f, CR.intrinsics(H, W, 60.0), [np.eye(4)], img[None])


def check_texture_beats_vertex_colours(side):
    """Known answer 4, the point of the feature: the mean absolute error of the textured render against the photograph is
    strictly below that of the vertex-colour render of the same mesh (nine colours cannot hold a checkerboard)."""
    s, S = checker_scene(), 8
    tex, used = side.bake(s, S, min_cos=0.0, fill=FILL)
    tex, _, _ = side.fill(tex, used, len(s["f"]), S, 2)
    image, fid = side.render(s, TR.corner_texels(len(s["f"]), S), tex)
    on = fid >= 0
    photo = s["imgs"][0].astype(np.float64)
    mae_t = np.abs(image[on] - photo[on]).mean()
    mae_v = np.abs(side.vertex_render(s)[on] - photo[on]).mean()
    print("checkerboard: mean absolute error textured %.2f, vertex colours %.2f, over %d pixels" % (mae_t, mae_v, on.sum()))
    assert on.sum() > 800 and mae_t < mae_v


def test_round_trip_reproduces_the_photograph():
    assert check_round_trip(NumpySide()) == 892                   # the square is 30 pixels across


def test_silhouette_fill():
    check_silhouette_fill(NumpySide())


def test_occlusion_and_fallback():
    check_occlusion_and_fallback(NumpySide())


def test_texture_beats_vertex_colours_on_a_checkerboard():
    check_texture_beats_vertex_colours(NumpySide())


# ------------------------------------------------------------------ the fill round
def test_fill_round_counts_only_neighbours_of_the_same_face():
    F, S = 2, 2                                                   # one cell of 5 x 5: even face i + j <= 4, odd the other ten
    face = TR.owner_map(F, S)[0]
    assert face.shape == (5, 5) and face[2, 2] == 0 and face[2, 3] == 1 and face[3, 2] == 1
    tex = np.zeros((5, 5, 3), np.uint8)
    state = np.zeros((5, 5), np.uint8)
    tex[2, 3], state[2, 3] = (200, 100, 50), 1                    # of the odd face, right of (2, 2)
    tex[2, 1], state[2, 1] = (10, 20, 31), 1                      # of the even face, left of (2, 2)
    tex[1, 2], state[1, 2] = (11, 20, 30), 1                      # of the even face, above (2, 2)
    t2, s2, filled = TR.fill_round(tex, state, F, S)
    assert tuple(t2[2, 2]) == (10, 20, 30) and s2[2, 2] == 1      # (10 + 11) / 2 = 10.5 -> 10 and (31 + 30) / 2 = 30.5 -> 30: half to even
    assert s2[3, 3] == 1 and tuple(t2[3, 3]) == (200, 100, 50)    # below (2, 3), odd like it
    assert s2[3, 2] == 0                                          # odd, its only coloured neighbour (2, 2) was empty in the in buffer


def test_fill_round_is_double_buffered_and_ends_after_an_empty_round():
    F, S = 1, 3                                                   # one face in a 6 x 6 cell; the odd half belongs to no face
    face = TR.owner_map(F, S)[0]
    tex = np.full((6, 6, 3), 9, np.uint8)
    used = np.zeros((6, 6), np.uint8)
    tex[0, 0], used[0, 0] = (100, 100, 100), 1
    t1, s1, filled = TR.fill_round(tex, used, F, S)
    assert filled == 2 and s1[0, 1] == 1 and s1[1, 0] == 1 and s1[1, 1] == 0 and s1[0, 2] == 0     # one texel a round
    assert np.array_equal(tex[0, 1], [9, 9, 9])                   # the in buffer is not written
    n_face = int((face == 0).sum())
    t, s, runs = TR.fill(tex, used, F, S, 100)
    assert (s[face == 0] == 1).all() and (t[face == 0] == 100).all()
    assert (s[face < 0] == 0).all() and (t[face < 0] == 9).all()  # texels of no face are copied, whatever the rounds
    assert runs == 5 + 1 and n_face == 21                       # the furthest texel (i + j = 5) is five steps away; the empty round counts
    assert TR.fill(tex, used, F, S, 3)[2] == 3 and TR.fill(tex, used, F, S, 0)[2] == 0
    assert TR.fill(tex, np.zeros_like(used), F, S, 7)[2] == 1     # nothing to start from: the first round is empty


# ------------------------------------------------------------------ header and binding
def test_lib_signatures_match_the_header():
    import ctypes as C

    from uforecon_amd import _lib
    from uforecon_amd.build import SOURCES

    text = open(os.path.join(ROOT, "include", "ufr.h")).read()
    assert text.count("/* ---- mesh texturing (ABI 507, additive) ----") == 1
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = []
    for res, name, params in re.findall(r"\b(int|size_t)\s+(ufr_texture_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        found.append(name)
        rtype, args = _lib.SIGNATURES[name]
        assert rtype is (C.c_size_t if res == "size_t" else C.c_int), name
        want = [p.strip() for p in params.split(",")]
        assert len(want) == len(args), name
        for p, a in zip(want, args):
            if "*" in p or p.startswith("ufr_stream"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}[p.split()[0]], (name, p)
    assert sorted(found) == ["ufr_texture_bake", "ufr_texture_fill_round", "ufr_texture_frames"]
    assert sorted(found) == sorted(n for n in _lib.SIGNATURES if n.startswith("ufr_texture_"))
    assert "mesh_texture.hip" in SOURCES
    assert "#define UFR_TEXTURE_MAX_PATCH %d" % TO.TEXTURE_MAX_PATCH in hdr and "#define UFR_TEXTURE_MAX_SIDE %d" % TO.TEXTURE_MAX_SIDE in hdr
    code = open(os.path.join(ROOT, "uforecon_amd", "csrc", "ufr_internal.h")).read()
    assert re.search(r"constexpr int kTextureThreads = (\d+);", code).group(1) == str(TO.TEXTURE_BLOCK)


def test_python_defaults_are_color_meshs_constants():
    p = inspect.signature(TM.texture_mesh).parameters
    assert (p["depth_tol"].default, p["min_cos"].default, p["power"].default, p["fill_color"].default) == \
        (CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER, CMesh.FILL_COLOR)
    assert (p["patch"].default, p["atlas_size"].default, p["mode"].default, p["fill_rounds"].default, p["vertex_fallback"].default,
            p["occlusion"].default, p["z_min"].default, p["return_timings"].default) == (None, 4096, "mean", 2, True, True, 0.0, False)
    b = inspect.signature(TO.mesh_texture_bake).parameters
    assert (b["depth_tol"].default, b["min_cos"].default, b["power"].default, b["fill"].default, b["mode"].default) == \
        (CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER, CMesh.FILL_COLOR, "mean")
    a = TM.make_parser().parse_args([])
    assert (a.depth_tol, a.min_cos, a.power, tuple(a.fill_color), a.fill_rounds, a.atlas_size, a.patch, a.mode) == \
        (CMesh.DEPTH_TOL, CMesh.MIN_COS, CMesh.POWER, CMesh.FILL_COLOR, 2, 4096, None, "mean")
    assert a.views == CM.TEST_REF_VIEW and not a.all_views and not a.no_vertex_fallback and not a.no_occlusion
    assert (TM.STATE_EMPTY, TM.STATE_SEEN, TM.STATE_FILLED, TM.STATE_FALLBACK, TM.STATE_NO_FACE) == (0, 1, 2, 3, 4)
    r = inspect.signature(RT.render_mesh).parameters
    assert r["texture"].default is None and r["corner_xy"].default is None
    assert RT.make_parser().parse_args(["--color", "texture"]).color == "texture"


# ------------------------------------------------------------------ files and the command
def test_obj_mtl_png_round_trip(tmp_path):
    v, f = CR.icosphere(1)
    v = (v * 123.456 + 7.0).astype(np.float32)
    S = 5
    xy = TO.corner_texels(len(f), S)
    Ht, Wt, _, _ = TO.atlas_layout(len(f), S)
    tex = np.random.default_rng(3).integers(0, 256, (Ht, Wt, 3)).astype(np.uint8)
    path = str(tmp_path / "scan7.obj")
    TM.write_obj(path, v, f, xy, tex)
    assert sorted(os.listdir(tmp_path)) == ["scan7.mtl", "scan7.obj", "scan7.png"]
    assert "map_Kd scan7.png" in open(tmp_path / "scan7.mtl").read()
    text = open(path).read()
    assert text.startswith("mtllib scan7.mtl\nusemtl scan7\nv ") and text.count("\nvt ") == 3 * len(f) and text.count("\nf ") == len(f)
    v2, f2, xy2, tex2 = TM.read_obj(path)
    assert v2.dtype == np.float32 and np.array_equal(v2.view(np.uint32), v.view(np.uint32))       # bit for bit
    assert f2.dtype == np.int32 and np.array_equal(f2, f) and np.array_equal(tex2, tex)
    u = (xy[..., 0] + 0.5) / Wt
    w = 1.0 - (xy[..., 1] + 0.5) / Ht
    uv2 = np.stack([(xy2[..., 0] + 0.5) / Wt, 1.0 - (xy2[..., 1] + 0.5) / Ht], -1)
    assert np.abs(uv2 - np.stack([u, w], -1)).max() <= 1e-12 and np.abs(xy2 - xy).max() < 1e-9
    line = [t for t in text.split("\n") if t.startswith("vt ")][0].split()
    assert float(line[1]) == u[0, 0] and float(line[2]) == w[0, 0]


def test_command_failures_are_one_line_each(tmp_path, capsys):
    """every failure below is met before any device work: this test runs without a GPU"""
    root, mesh_dir, out_dir = str(tmp_path / "dtu"), str(tmp_path / "mesh"), str(tmp_path / "out")
    os.makedirs(mesh_dir)
    v, f = CR.icosphere(0)
    H, W = 6, 8
    rng = np.random.default_rng(0)
    pics = {s: [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)] for s in (1, 2, 3, 4)}
    pics[3][1] = rng.integers(0, 256, (H + 2, W, 3)).astype(np.uint8)
    CR.write_dtu_tree(root, [1, 2, 3, 4], [5, 6], CR.intrinsics(H, W, 10.0), CR.ring_cameras(2, 4.0), pics)
    for s in (1, 2, 3):
        CM.write_ply(os.path.join(mesh_dir, "scan%d.ply" % s), v, f)
    CM.write_ply(os.path.join(mesh_dir, "scan4.ply"), v, np.zeros((0, 3), np.int32))
    os.remove(os.path.join(root, "scan1", "image", "000006.png"))
    common = ["--mesh_dir", mesh_dir, "--root_dir", root, "--out_dir", out_dir]
    assert TM.main(common + ["--scans", "1", "3", "4", "9", "--views", "5", "6"]) == 0
    assert TM.main(common + ["--scans", "2", "--views", "5", "7"]) == 0
    assert TM.main(common + ["--scans", "2", "--views", "5", "6", "--atlas_size", "15"]) == 0     # 20 faces: 4 x 3 cells of >= 4 texels
    assert TM.main(common + ["--scans", "2", "--views", "5", "6", "--patch", "126"]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 7
    assert lines[0].startswith("scan1: no picture at ") and lines[0].endswith("000006.png")
    assert lines[1].startswith("scan3: pictures of unequal size")
    assert lines[2].startswith("scan4: ") and lines[2].endswith("has no faces")
    assert lines[3].startswith("scan9: no mesh at ")
    assert lines[4].startswith("scan2: no camera at ") and lines[4].endswith("00000007_cam.txt")
    assert lines[5].startswith("scan2: the atlas does not fit: ") and lines[6].startswith("scan2: the atlas does not fit: ")
    assert json.load(open(os.path.join(out_dir, "texture_mesh.json"))) == {}
    assert not [p for p in os.listdir(out_dir) if p.endswith((".obj", ".mtl", ".png"))]
