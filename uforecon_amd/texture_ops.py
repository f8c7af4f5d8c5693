"""Torch-facing wrappers of mesh texturing (include/ufr.h, "mesh texturing"; csrc/mesh_texture.hip), in the idiom of ops.py:
torch owns device memory and the current stream, every computation is a libufr.so kernel, and every wrapper validates device,
dtype and contiguity and raises ``UfrError`` with the library's message on failure.  uforecon_amd/texture_mesh.py strings these
together; tests/texture_ref.py restates them in numpy.  The atlas is a closed form of (F, S), stated here on the host
(``atlas_layout``, ``corner_texels``) and in the library on the device.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import UfrError
from .ops import MESH_COLOR_MAX_POWER, MESH_COLOR_MODES, MESH_MAX_VIEWS, _dev, _points64, _stream

TEXTURE_BLOCK = 256              # kTextureThreads of csrc/ufr_internal.h: the texels one block owns
TEXTURE_MAX_PATCH = 125          # UFR_TEXTURE_MAX_PATCH of include/ufr.h
TEXTURE_MAX_SIDE = 16384         # UFR_TEXTURE_MAX_SIDE


# ---- the atlas (host side of the closed form)
def atlas_layout(F: int, S: int):
    """``(Ht, Wt, cols, rows)`` of the atlas of ``F`` faces at patch size ``S``: cells of side S + 3, faces 2q and 2q + 1 in
    cell q, cols = ceil(sqrt(cells)) in integers.  Raises when S is outside 1..125, F < 1 or a side exceeds 16384."""
    F, S = int(F), int(S)
    if not 1 <= S <= TEXTURE_MAX_PATCH:
        raise UfrError(f"atlas_layout: S {S} (must be 1 .. {TEXTURE_MAX_PATCH})")
    if not 1 <= F < 2 ** 31:
        raise UfrError(f"atlas_layout: F {F} (must be 1 .. 2^31 - 1)")
    cells = (F + 1) // 2
    cols = math.isqrt(cells - 1) + 1                # ceil(sqrt(cells)), exact
    rows = (cells + cols - 1) // cols
    side = S + 3
    Ht, Wt = rows * side, cols * side
    if Ht > TEXTURE_MAX_SIDE or Wt > TEXTURE_MAX_SIDE:
        raise UfrError(f"atlas_layout: {F} faces at S {S} need an atlas of {Wt}x{Ht} (a side above {TEXTURE_MAX_SIDE})")
    return Ht, Wt, cols, rows


def corner_texels(F: int, S: int):
    """(F,3,2) float64: the texel coordinates (x, y) of every face's corners a, b, c in the atlas of ``atlas_layout(F, S)`` --
    even face: (0,0), (S,0), (0,S) of its cell; odd face: (C-1,C-1), (C-1-S,C-1), (C-1,C-1-S), a half turn"""
    import numpy as np

    _, _, cols, _ = atlas_layout(F, S)
    S, side = int(S), int(S) + 3
    f = np.arange(int(F), dtype=np.int64)
    q = f // 2
    ox, oy = (q % cols) * side, (q // cols) * side
    even = np.array([[0, 0], [S, 0], [0, S]], np.int64)
    odd = side - 1 - even
    local = np.where((f % 2 == 0)[:, None, None], even[None], odd[None])
    return (local + np.stack([ox, oy], 1)[:, None, :]).astype(np.float64)


def patch_for_atlas(F: int, atlas_size: int) -> int:
    """The largest S in 1..125 whose atlas for ``F`` faces fits ``atlas_size`` x ``atlas_size`` texels; raises when S = 1 does
    not.  Ht and Wt grow with S, so the first S that does not fit ends the search."""
    F, atlas_size = int(F), int(atlas_size)
    if not 1 <= atlas_size <= TEXTURE_MAX_SIDE:
        raise UfrError(f"patch_for_atlas: atlas_size {atlas_size} (must be 1 .. {TEXTURE_MAX_SIDE})")
    if not 1 <= F < 2 ** 31:
        raise UfrError(f"patch_for_atlas: F {F} (must be 1 .. 2^31 - 1)")
    cells = (F + 1) // 2
    cols = math.isqrt(cells - 1) + 1
    rows = (cells + cols - 1) // cols               # rows <= cols
    best = min(atlas_size // cols - 3, TEXTURE_MAX_PATCH)
    if best < 1:
        raise UfrError(f"patch_for_atlas: {F} faces need {cols} x {rows} cells of at least 4 texels: more than {atlas_size} x "
                       f"{atlas_size}")
    return best


def _atlas(S, Ht, Wt, F, who: str):
    lay = atlas_layout(F, S)
    if (int(Ht), int(Wt)) != lay[:2]:
        raise UfrError(f"{who}: atlas {Wt}x{Ht} is not the closed form for F {F}, S {S}: {lay[1]}x{lay[0]}")
    return lay


# ---- the kernels
def mesh_texture_bake(verts: torch.Tensor, faces: torch.Tensor, images: torch.Tensor, depth: Optional[torch.Tensor], k, w2c, centre,
                      S: int, z_min: float = 0.0, depth_tol: float = 0.005, min_cos: float = 0.2, power: int = 2,
                      mode: str = "mean", fill=(128, 128, 128), fallback: Optional[torch.Tensor] = None):
    """ufr_texture_bake: the atlas of ``atlas_layout(F, S)`` baked from ``n`` photographs, one thread per texel (include/ufr.h
    states every rule).  ``verts`` (V,3) CUDA float64, ``faces`` (F,3) CUDA int32; ``images``, ``depth``, ``k``, ``w2c``,
    ``centre`` and the thresholds as ``ops.mesh_vertex_colors`` takes them; ``fallback`` (V,3) CUDA uint8 vertex colours or
    None: what a texel no view saw interpolates (else ``fill``).  Returns ``texture`` (Ht,Wt,3) uint8 and ``views_used``
    (Ht,Wt) uint8.  A face index out of range is not an error: that face's texels get ``fill``.  Synchronises nowhere."""
    import numpy as np

    pv = _points64(verts, "verts")
    pf = _dev(faces, "faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise UfrError(f"faces: expected shape (F, 3), got {tuple(faces.shape)}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V < 1 or F < 1:
        raise UfrError(f"mesh_texture_bake: the mesh has {V} vertices and {F} faces (need at least one of each)")
    Ht, Wt, _, _ = atlas_layout(F, S)
    pi = _dev(images, "images", torch.uint8)
    if images.dim() != 4 or images.shape[3] != 3:
        raise UfrError(f"images: expected shape (n, H, W, 3), got {tuple(images.shape)}")
    n, H, W = (int(s) for s in images.shape[:3])
    if not 1 <= n <= MESH_MAX_VIEWS:
        raise UfrError(f"mesh_texture_bake: {n} views (must be 1 .. {MESH_MAX_VIEWS})")
    if H < 2 or W < 2 or H * W >= 2 ** 31:
        raise UfrError(f"mesh_texture_bake: image {H}x{W} (H, W >= 2, H * W < 2^31)")
    pd = pb = None
    if depth is not None:
        pd = _dev(depth, "depth", torch.float32)
        if tuple(depth.shape) != (n, H, W):
            raise UfrError(f"depth: expected shape ({n}, {H}, {W}), got {tuple(depth.shape)}")
    if fallback is not None:
        pb = _dev(fallback, "fallback", torch.uint8)
        if tuple(fallback.shape) != (V, 3):
            raise UfrError(f"fallback: expected shape ({V}, 3), got {tuple(fallback.shape)}")
    kk = np.ascontiguousarray(np.asarray(k, np.float64))
    wc = np.ascontiguousarray(np.asarray(w2c, np.float64))
    cc = np.ascontiguousarray(np.asarray(centre, np.float64))
    if kk.shape != (n, 3, 3) or wc.shape != (n, 4, 4) or cc.shape != (n, 3):
        raise UfrError(f"mesh_texture_bake: k {kk.shape}, w2c {wc.shape}, centre {cc.shape}: expected ({n}, 3, 3), ({n}, 4, 4) "
                       f"and ({n}, 3)")
    if int(power) != power or not 0 <= int(power) <= MESH_COLOR_MAX_POWER:
        raise UfrError(f"mesh_texture_bake: power {power} (an integer in 0 .. {MESH_COLOR_MAX_POWER})")
    if mode not in MESH_COLOR_MODES:
        raise UfrError(f"mesh_texture_bake: mode {mode!r} (one of {sorted(MESH_COLOR_MODES)})")
    fl = np.ascontiguousarray(np.asarray(fill).reshape(-1))
    if fl.shape != (3,) or not ((fl >= 0) & (fl <= 255) & (fl == np.rint(fl))).all():
        raise UfrError(f"mesh_texture_bake: fill {fill!r} (three integers in 0 .. 255)")
    fl = np.ascontiguousarray(fl.astype(np.uint8))
    dev = verts.device
    texture = torch.empty((Ht, Wt, 3), dtype=torch.uint8, device=dev)
    used = torch.empty((Ht, Wt), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    nbytes = lib.ufr_color_vertices_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dp = C.POINTER(C.c_double)
    _lib.check(lib.ufr_texture_bake(pv, pf, V, F, pi, pd, kk.ctypes.data_as(dp), wc.ctypes.data_as(dp), cc.ctypes.data_as(dp), n, H, W,
                                    int(S), Ht, Wt, float(z_min), float(depth_tol), float(min_cos), int(power),
                                    MESH_COLOR_MODES[mode], fl.ctypes.data_as(C.POINTER(C.c_uint8)), pb, texture.data_ptr(),
                                    used.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ufr_texture_bake")
    return texture, used


def mesh_texture_fill(texture: torch.Tensor, views_used: torch.Tensor, S: int, F: int, rounds: int):
    """Up to ``rounds`` rounds of ufr_texture_fill_round: a texel without colour (``views_used`` == 0) of some face takes the
    mean of its coloured 4-neighbours of the same face, rounded half to even; one round reaches one texel further.
    ``texture`` (Ht,Wt,3) CUDA uint8, ``views_used`` (Ht,Wt) CUDA uint8, the atlas of ``atlas_layout(F, S)``.  Returns
    ``texture`` (Ht,Wt,3) uint8, ``state`` (Ht,Wt) uint8 (0: still empty) and the rounds run -- a round that fills nothing is
    the last, and is counted.  One host read per round."""
    _dev(texture, "texture", torch.uint8)
    _dev(views_used, "views_used", torch.uint8)
    if texture.dim() != 3 or texture.shape[2] != 3 or tuple(views_used.shape) != tuple(texture.shape[:2]):
        raise UfrError(f"mesh_texture_fill: texture {tuple(texture.shape)}, views_used {tuple(views_used.shape)}: expected "
                       "(Ht, Wt, 3) and (Ht, Wt)")
    Ht, Wt = int(texture.shape[0]), int(texture.shape[1])
    S, F = int(S), int(F)
    _atlas(S, Ht, Wt, F, "mesh_texture_fill")
    rounds = int(rounds)
    if rounds < 0:
        raise UfrError(f"mesh_texture_fill: rounds {rounds} (must be >= 0)")
    cur, state = texture.clone(), (views_used != 0).to(torch.uint8)
    if rounds == 0:
        return cur, state, 0
    nxt, nstate = torch.empty_like(cur), torch.empty_like(state)
    filled = torch.zeros(1, dtype=torch.int32, device=texture.device)
    lib, run = _lib.load(), 0
    while run < rounds:
        filled.zero_()
        _lib.check(lib.ufr_texture_fill_round(cur.data_ptr(), state.data_ptr(), S, Ht, Wt, F, nxt.data_ptr(), nstate.data_ptr(),
                                              filled.data_ptr(), _stream()), "ufr_texture_fill_round")
        cur, nxt, state, nstate = nxt, cur, nstate, state
        run += 1
        if int(filled.item()) == 0:
            break
    return cur, state, run


def raster_frames_textured(verts: torch.Tensor, faces: torch.Tensor, k_inv, c2ws, H: int, W: int, corner_xy: torch.Tensor,
                           texture: torch.Tensor, normals: Optional[torch.Tensor] = None, background=(255, 255, 255),
                           ambient: float = 0.25, return_depth: bool = False, return_face_ids: bool = False,
                           return_normals: bool = False, check_indices: bool = True):
    """ufr_texture_frames: ``ops.raster_frames`` with the colour of a pixel taken from ``texture`` (Ht,Wt,3) CUDA uint8 at the
    barycentric mix of its face's corner texels ``corner_xy`` (F,3,2) CUDA float64, sampled bilinearly with the indices
    clamped to the texture (include/ufr.h states every rule).  The other arguments, the returned dict and the synchronisation
    are those of ``ops.raster_frames``.  No mipmaps: render larger and ``ops.raster_downsample`` for antialiasing."""
    import numpy as np

    from .ops import _mesh

    if check_indices:
        pv, pf, V, F = _mesh(verts, faces, "raster_frames_textured")
    else:
        pv, pf, V, F = _points64(verts, "verts"), _dev(faces, "faces", torch.int32), int(verts.shape[0]), int(faces.shape[0])
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise UfrError(f"faces: expected shape (F, 3), got {tuple(faces.shape)}")
    pxy = _dev(corner_xy, "corner_xy", torch.float64)
    if tuple(corner_xy.shape) != (F, 3, 2):
        raise UfrError(f"corner_xy: expected shape ({F}, 3, 2), got {tuple(corner_xy.shape)}")
    pt = _dev(texture, "texture", torch.uint8)
    if texture.dim() != 3 or texture.shape[2] != 3 or not 1 <= texture.shape[0] <= TEXTURE_MAX_SIDE \
            or not 1 <= texture.shape[1] <= TEXTURE_MAX_SIDE:
        raise UfrError(f"texture: expected shape (Ht, Wt, 3) with Ht, Wt in 1 .. {TEXTURE_MAX_SIDE}, got {tuple(texture.shape)}")
    Ht, Wt = int(texture.shape[0]), int(texture.shape[1])
    ki = np.ascontiguousarray(np.asarray(k_inv, np.float32))
    cw = np.ascontiguousarray(np.asarray(c2ws, np.float32))
    if ki.shape != (3, 3) or cw.ndim != 3 or cw.shape[1:] != (4, 4) or cw.shape[0] < 1:
        raise UfrError(f"raster_frames_textured: k_inv {ki.shape}, c2ws {cw.shape}: expected (3, 3) and (n, 4, 4) with n >= 1")
    n, H, W = int(cw.shape[0]), int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise UfrError(f"raster_frames_textured: image {H}x{W} (H, W >= 1, H * W < 2^31)")
    if not 0.0 <= float(ambient) <= 1.0:
        raise UfrError(f"raster_frames_textured: ambient {ambient} (must be 0 .. 1)")
    bg = np.ascontiguousarray(np.asarray(background).reshape(-1))
    if bg.shape != (3,) or not ((bg >= 0) & (bg <= 255) & (bg == np.rint(bg))).all():
        raise UfrError(f"raster_frames_textured: background {background!r} (three integers in 0 .. 255)")
    bg = np.ascontiguousarray(bg.astype(np.uint8))
    pn = None
    if normals is not None:
        pn = _points64(normals, "normals")
        if normals.shape[0] != V:
            raise UfrError(f"normals: expected shape ({V}, 3), got {tuple(normals.shape)}")
    dev = verts.device
    bgt = torch.from_numpy(bg).to(dev)
    out = {"image": bgt.expand(n, H, W, 3).contiguous()}
    if return_depth:
        out["depth"] = torch.zeros((n, H, W), dtype=torch.float32, device=dev)
    if return_face_ids:
        out["face_id"] = torch.full((n, H, W), -1, dtype=torch.int32, device=dev)
    if return_normals:
        out["normal"] = torch.zeros((n, H, W, 3), dtype=torch.float32, device=dev)
    if F == 0 or V == 0:
        return out
    lib = _lib.load()
    nbytes = lib.ufr_raster_frames_workspace_bytes(F, H, W)
    if nbytes == 0:
        raise UfrError(f"raster_frames_textured: F {F}, image {H}x{W} unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fp, ptr = C.POINTER(C.c_float), lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    _lib.check(lib.ufr_texture_frames(pv, pf, V, F, pn, pxy, pt, Ht, Wt, ki.ctypes.data_as(fp), cw.ctypes.data_as(fp), n, H, W,
                                      bg.ctypes.data_as(C.POINTER(C.c_uint8)), float(ambient), out["image"].data_ptr(), ptr("depth"),
                                      ptr("face_id"), ptr("normal"), ws.data_ptr(), nbytes, _stream()), "ufr_texture_frames")
    return out
