"""Mesh texturing on the GPU: a per-face texture atlas baked from the photographs -- what a mesh thinned by ``simplify_mesh``
needs to carry the pictures' detail, which ``color_mesh``'s one colour per vertex cannot.  Its hot loop is a HIP kernel
(csrc/mesh_texture.hip through ``texture_ops.mesh_texture_bake`` and ``texture_ops.mesh_texture_fill``); include/ufr.h states
every rule, tests/texture_ref.py restates them in numpy.  The reference has no such stage.

    python -m uforecon_amd.texture_mesh --mesh_dir OUT/mesh/simple --root_dir DTU_TEST --out_dir OUT/mesh/texture
        [--views 23 24 33 ... | --all_views] [--patch S | --atlas_size N] [--mode mean|best] [--depth_tol T] [--min_cos C]
        [--power P] [--fill_rounds 2] [--no_vertex_fallback] [--fill_color r g b] [--no_occlusion] [--scans ...] [--ply FILE ...]

reads ``<mesh_dir>/scan<N>.ply`` and the cameras and pictures ``color_mesh`` reads, writes ``<out_dir>/scan<N>.obj``,
``scan<N>.mtl``, ``scan<N>.png`` and ``<out_dir>/texture_mesh.json`` (texel counts per state, the atlas size, S, the
milliseconds of every stage).  ``render_trajectory --color texture`` draws the result.

1. the atlas: every face gets a right-angled patch of S texel steps a leg, two faces a square cell, in closed form
   (``texture_ops.atlas_layout``); S is ``--patch`` or the largest that fits ``--atlas_size``;
2. per view the mesh's own z-depth at the picture's size, as ``color_mesh`` makes it;
3. every texel is placed on its face, projected into every view in fp64 and put through ``color_mesh``'s per-view rule
   (depth test over the four texels of the footprint, viewing angle against the face normal, cos^power blend);
4. texels no view saw interpolate the vertex colours of ``color_mesh`` (``--no_vertex_fallback``: the fill colour);
5. two rounds of a texel-space neighbour fill close the gutter that projects outside a picture at a silhouette.

Not done: charts and patch sizes by face area (uniform S suits marching-cubes and clustered meshes), per-face view selection,
seam levelling, exposure compensation, mipmaps (``render_trajectory --supersample`` is the antialiasing), a custom-scene
command.  Open3D and MVS-texturing were not compared against, and no real scan has been textured.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

from .clean_mesh import TEST_REF_VIEW, ray_camera, read_cam_file
from .color_mesh import ALL_VIEWS, DEPTH_TOL, FILL_COLOR, FILL_ROUNDS as VERTEX_FILL_ROUNDS, MIN_COS, POWER, projection_camera, read_image
from .dtu_eval import DTU_SCANS, read_ply

ATLAS_SIZE = 4096                                # a stated choice, not tuned: 16.8 M texels, 50 MB as RGB
FILL_ROUNDS = 2                                  # the gutter's depth: up to two texels past a patch's hypotenuse
STATE_EMPTY, STATE_SEEN, STATE_FILLED, STATE_FALLBACK, STATE_NO_FACE = 0, 1, 2, 3, 4
STATE_NAMES = ("empty", "seen", "filled", "fallback", "no_face")


def texture_mesh(verts, faces, cams, images, patch=None, atlas_size=ATLAS_SIZE, mode="mean", depth_tol=DEPTH_TOL, min_cos=MIN_COS,
                 power=POWER, fill_rounds=FILL_ROUNDS, vertex_fallback=True, fill_color=FILL_COLOR, occlusion=True, z_min=0.0,
                 return_timings=False, device="cuda"):
    """A texture atlas of a mesh from photographs, in memory.  ``verts`` (V,3) any float dtype (widened to float64 once),
    ``faces`` (F,3) integers; ``cams`` and ``images`` as ``color_mesh.color_mesh`` takes them.  ``patch``: S, or None for the
    largest that fits ``atlas_size`` squared.  Returns numpy arrays: ``texture`` (Ht,Wt,3) uint8, ``corner_xy`` (F,3,2) float64
    (texel coordinates of every face's corners), ``views_used`` (Ht,Wt) uint8 and ``state`` (Ht,Wt) uint8 -- ``STATE_SEEN``:
    coloured by a view, ``STATE_FILLED``: by its neighbours, ``STATE_FALLBACK``: from the vertex colours, ``STATE_EMPTY``:
    ``fill_color``, ``STATE_NO_FACE``: outside every patch; with ``return_timings`` also a dict of milliseconds per stage.

    With ``vertex_fallback`` the vertex colours are ``ops.mesh_vertex_colors`` with the area-weighted vertex normals, then
    ``ops.mesh_color_fill`` with ``color_mesh``'s round count: what ``color_mesh`` would give the same mesh."""
    import torch

    from . import ops, texture_ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    cams, images = list(cams), [np.asarray(m) for m in images]
    if len(cams) != len(images) or not cams:
        raise UfrError(f"texture_mesh: {len(cams)} cameras, {len(images)} pictures (need one picture per camera, at least one)")
    if len(cams) > ops.MESH_MAX_VIEWS:
        raise UfrError(f"texture_mesh: {len(cams)} views (at most {ops.MESH_MAX_VIEWS})")
    for m in images:
        if m.ndim != 3 or m.shape[2] != 3 or m.dtype != np.uint8 or m.shape != images[0].shape:
            raise UfrError(f"texture_mesh: pictures must be (H, W, 3) uint8 of one size, got {[(x.shape, str(x.dtype)) for x in images]}")
    V, F = len(verts), len(faces)
    if F == 0 or V == 0:
        raise UfrError(f"texture_mesh: the mesh has {V} vertices and {F} faces (need at least one face)")
    if faces.min() < 0 or faces.max() >= V:                        # the one index check: every call below trusts it
        raise UfrError(f"texture_mesh: face indices span {faces.min()}..{faces.max()}, the mesh has {V} vertices")
    S = texture_ops.patch_for_atlas(F, atlas_size) if patch is None else int(patch)
    Ht, Wt, _, _ = texture_ops.atlas_layout(F, S)                 # before any device work: an atlas that does not fit raises here
    corner_xy = texture_ops.corner_texels(F, S)
    dev = torch.device(device)
    n, (H, W) = len(cams), images[0].shape[:2]
    ms, t0 = {}, [0.0]

    def tick():
        torch.cuda.synchronize(dev)
        t0[0] = time.perf_counter()

    def tock(name):
        torch.cuda.synchronize(dev)
        ms[name] = (time.perf_counter() - t0[0]) * 1e3

    tick()
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(dev)
    ti = torch.from_numpy(np.ascontiguousarray(np.stack(images))).to(dev)
    tock("upload_ms")
    tick()
    depth = None
    if occlusion:
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        for i, (K, E) in enumerate(cams):
            k_inv, c2w = ray_camera(K, E)
            depth[i] = ops.raster_frames(tv, tf, k_inv, c2w[None], H, W, return_depth=True, check_indices=False)["depth"][0]
    tock("depth_ms")
    pk, pw, pc = (np.stack(a) for a in zip(*[projection_camera(K, E) for K, E in cams]))
    rule = dict(z_min=z_min, depth_tol=depth_tol, min_cos=min_cos, power=power, mode=mode)
    tick()
    fallback = None
    if vertex_fallback:
        tn = ops.raster_vertex_normals(tv, tf)
        vcol, vused = ops.mesh_vertex_colors(tv, tn, ti, depth, pk, pw, pc, fill=fill_color, **rule)
        fallback, _, _ = ops.mesh_color_fill(tf, vcol, vused, VERTEX_FILL_ROUNDS)
    tock("fallback_ms")
    tick()
    tex, used = texture_ops.mesh_texture_bake(tv, tf, ti, depth, pk, pw, pc, S, fill=fill_color, fallback=fallback, **rule)
    tock("bake_ms")
    tick()
    tex, has, rounds_run = texture_ops.mesh_texture_fill(tex, used, S, F, fill_rounds)
    tock("fill_ms")
    used = used.cpu().numpy()
    state = np.where(used > 0, STATE_SEEN, np.where(has.cpu().numpy() != 0, STATE_FILLED,
                                                    STATE_FALLBACK if vertex_fallback else STATE_EMPTY)).astype(np.uint8)
    state[~texel_has_face(F, S)] = STATE_NO_FACE
    ms["fill_rounds_run"] = rounds_run
    out = (tex.cpu().numpy(), corner_xy, used, state)
    return out + (ms,) if return_timings else out


def texel_has_face(F, S):
    """(Ht,Wt) bool: the texels of the atlas of ``texture_ops.atlas_layout(F, S)`` that belong to a face (patch or gutter)"""
    from . import texture_ops

    Ht, Wt, cols, _ = texture_ops.atlas_layout(F, S)
    side = int(S) + 3
    ys, xs = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    q = (ys // side) * cols + xs // side
    odd = (xs % side) + (ys % side) > int(S) + 2
    return 2 * q + odd < int(F)


# ------------------------------------------------------------------ files
def write_obj(filename, verts, faces, corner_xy, texture):
    """``filename`` (.obj) with ``v`` lines (%.9g: a float32 survives), three ``vt`` per face -- u = (x + 0.5) / Wt, v = 1 -
    (y + 0.5) / Ht: texel centres are the integers, OBJ's v axis points up -- and ``f a/ta b/tb c/tc``; beside it the ``.mtl``
    (one material, ``map_Kd``) and the texture as ``.png``, both named after the file."""
    from PIL import Image

    verts = np.asarray(verts).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    corner_xy = np.asarray(corner_xy, np.float64)
    texture = np.asarray(texture)
    if corner_xy.shape != (len(faces), 3, 2):
        raise ValueError(f"write_obj: corner_xy {corner_xy.shape}: expected {(len(faces), 3, 2)}")
    if texture.ndim != 3 or texture.shape[2] != 3 or texture.dtype != np.uint8:
        raise ValueError(f"write_obj: texture {texture.shape} {texture.dtype}: expected (Ht, Wt, 3) uint8")
    Ht, Wt = texture.shape[:2]
    stem = os.path.splitext(filename)[0]
    name = os.path.basename(stem)
    Image.fromarray(texture).save(stem + ".png")
    with open(stem + ".mtl", "w") as f:
        f.write("newmtl %s\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s.png\n" % (name, name))
    uv = np.stack([(corner_xy[..., 0] + 0.5) / Wt, 1.0 - (corner_xy[..., 1] + 0.5) / Ht], -1).reshape(-1, 2)
    lines = ["mtllib %s.mtl" % name, "usemtl %s" % name]
    lines += ["v %.9g %.9g %.9g" % tuple(float(c) for c in p) for p in verts]
    lines += ["vt %.17g %.17g" % (float(u), float(v)) for u, v in uv]
    lines += ["f %d/%d %d/%d %d/%d" % (a + 1, 3 * i + 1, b + 1, 3 * i + 2, c + 1, 3 * i + 3) for i, (a, b, c) in enumerate(faces.tolist())]
    with open(filename, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_obj(filename):
    """What ``write_obj`` wrote: ``verts`` (V,3) float32, ``faces`` (F,3) int32, ``corner_xy`` (F,3,2) float64 in texels (the
    inverse of the uv rule, so within an ulp or two of what was written) and ``texture`` (Ht,Wt,3) uint8 from the material's
    ``map_Kd``.  Only triangles with ``v/vt`` corners are read."""
    v, vt, fv, ft, mtl = [], [], [], [], None
    with open(filename) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(t) for t in p[1:4]])
            elif p[0] == "vt":
                vt.append([float(t) for t in p[1:3]])
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"{filename}: a face with {len(p) - 1} corners (triangles only)")
                ids = [t.split("/") for t in p[1:4]]
                if any(len(t) < 2 or not t[1] for t in ids):
                    raise ValueError(f"{filename}: a face without texture coordinates")
                fv.append([int(t[0]) - 1 for t in ids])
                ft.append([int(t[1]) - 1 for t in ids])
            elif p[0] == "mtllib":
                mtl = p[1]
    if mtl is None:
        raise ValueError(f"{filename} names no material file")
    here, tex_name = os.path.dirname(filename), None
    with open(os.path.join(here, mtl)) as f:
        for line in f:
            p = line.split()
            if p and p[0] == "map_Kd":
                tex_name = p[1]
    if tex_name is None:
        raise ValueError(f"{os.path.join(here, mtl)} names no map_Kd")
    texture = read_image(os.path.join(here, tex_name))
    Ht, Wt = texture.shape[:2]
    verts = np.asarray(v, np.float64).reshape(-1, 3).astype(np.float32)
    faces = np.asarray(fv, np.int32).reshape(-1, 3)
    uv = np.asarray(vt, np.float64).reshape(-1, 2)[np.asarray(ft, np.int64).reshape(-1, 3)]
    corner_xy = np.stack([uv[..., 0] * Wt - 0.5, (1.0 - uv[..., 1]) * Ht - 0.5], -1)
    return verts, faces, corner_xy, texture


# ------------------------------------------------------------------ the command
def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh_dir", type=str, default="./outputs/mesh/simple", help="directory of scan<N>.ply")
    parser.add_argument("--root_dir", type=str, default="./dtu_test", help="dataset (cameras/<view>_cam.txt, scan<N>/image/<view>.png)")
    parser.add_argument("--out_dir", type=str, default="./outputs/mesh/texture", help="scan<N>.obj / .mtl / .png and texture_mesh.json go here")
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    group = parser.add_mutually_exclusive_group()
    group.add_argument("--views", type=int, nargs="+", default=TEST_REF_VIEW, help="the photographs to texture from")
    group.add_argument("--all_views", action="store_true", help="all 49 photographs of a DTU scan")
    parser.add_argument("--ply", type=str, nargs="+", default=None,
                        help="texture these mesh files instead of scan<N>.ply, paired in order with --scans, each to <out_dir>/<file stem>.obj")
    size = parser.add_mutually_exclusive_group()
    size.add_argument("--patch", type=int, default=None, help="S: texel steps along a triangle's legs (1 .. 125)")
    size.add_argument("--atlas_size", type=int, default=ATLAS_SIZE, help="the largest S whose atlas fits this many texels squared")
    parser.add_argument("--mode", choices=["mean", "best"], default="mean", help="blend the views by cos^power, or take the most frontal")
    parser.add_argument("--depth_tol", type=float, default=DEPTH_TOL, help="relative depth slack of the occlusion test")
    parser.add_argument("--min_cos", type=float, default=MIN_COS, help="views at a flatter angle than this cosine are not used")
    parser.add_argument("--power", type=int, default=POWER, help="weight of a view: cos^power (0 .. 8)")
    parser.add_argument("--fill_rounds", type=int, default=FILL_ROUNDS, help="texel-space neighbour-fill rounds (2: the gutter's depth)")
    parser.add_argument("--no_vertex_fallback", action="store_true", help="texels no view saw get the fill colour, not the vertex colours")
    parser.add_argument("--fill_color", type=int, nargs=3, default=list(FILL_COLOR), help="colour of the texels left empty")
    parser.add_argument("--no_occlusion", action="store_true", help="skip the depth maps: every view that contains a texel colours it")
    return parser


def texture_scan(mesh_path, root_dir, scan, views, out_path, patch=None, atlas_size=ATLAS_SIZE, **kw):
    """One scan: textures ``mesh_path`` from the pictures ``views`` of ``scan`` and writes ``out_path`` (.obj) with its .mtl and
    .png.  Returns the report dict of ``texture_mesh.json``.  Raises ValueError with one line for a missing picture or camera,
    pictures of unequal size, a mesh without faces and an atlas that does not fit -- all before any device work."""
    from . import texture_ops
    from ._lib import UfrError

    verts, faces = read_ply(mesh_path)
    if faces is None or len(faces) == 0:
        raise ValueError(f"{mesh_path} has no faces")
    try:
        S = texture_ops.patch_for_atlas(len(faces), atlas_size) if patch is None else int(patch)
        Ht, Wt, _, _ = texture_ops.atlas_layout(len(faces), S)
    except UfrError as e:
        raise ValueError(f"the atlas does not fit: {e}")
    cams, images = [], []
    for v in views:
        cam = os.path.join(root_dir, "cameras/{:0>8}_cam.txt".format(v))
        img = os.path.join(root_dir, "scan{}/image/{:0>6}.png".format(scan, v))
        for p, what in ((cam, "camera"), (img, "picture")):
            if not os.path.exists(p):
                raise ValueError(f"no {what} at {p}")
        cams.append(read_cam_file(cam))
        images.append(read_image(img))
        if images[-1].shape != images[0].shape:
            raise ValueError(f"pictures of unequal size: {img} is {images[-1].shape[1]}x{images[-1].shape[0]}, "
                             f"the first is {images[0].shape[1]}x{images[0].shape[0]}")
    texture, corner_xy, used, state, ms = texture_mesh(verts, faces, cams, images, patch=S, return_timings=True, **kw)
    write_obj(out_path, verts, faces, corner_xy, texture)
    counts = np.bincount(state.reshape(-1), minlength=len(STATE_NAMES))
    return dict(mesh=mesh_path, views=[int(v) for v in views], vertices=int(len(verts)), faces=int(len(faces)), patch=int(S),
                atlas=[int(Wt), int(Ht)], texels={name: int(c) for name, c in zip(STATE_NAMES, counts)}, **ms)


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    views = ALL_VIEWS if args.all_views else args.views
    if args.ply is not None and len(args.ply) != len(args.scans):
        parser.error(f"--ply names {len(args.ply)} files, --scans {len(args.scans)} scans: they are paired in order")
    if args.ply is not None:
        jobs = [(os.path.splitext(os.path.basename(p))[0], p, scan) for p, scan in zip(args.ply, args.scans)]
    else:
        jobs = [("scan%d" % scan, os.path.join(args.mesh_dir, "scan%d.ply" % scan), scan) for scan in args.scans]
    os.makedirs(args.out_dir, exist_ok=True)
    report = {}
    for name, path, scan in jobs:
        if not os.path.exists(path):
            print("%s: no mesh at %s" % (name, path))
            continue
        try:
            report[name] = texture_scan(path, args.root_dir, scan, views, os.path.join(args.out_dir, name + ".obj"), patch=args.patch,
                                        atlas_size=args.atlas_size, mode=args.mode, depth_tol=args.depth_tol, min_cos=args.min_cos,
                                        power=args.power, fill_rounds=args.fill_rounds, vertex_fallback=not args.no_vertex_fallback,
                                        fill_color=tuple(args.fill_color), occlusion=not args.no_occlusion)
        except ValueError as e:
            print("%s: %s" % (name, e))
            continue
        r = report[name]
        print("%s: %d faces, S %d, atlas %dx%d, %d texels seen, %d filled, %d from vertex colours, %d left empty"
              % (name, r["faces"], r["patch"], r["atlas"][0], r["atlas"][1], r["texels"]["seen"], r["texels"]["filled"],
                 r["texels"]["fallback"], r["texels"]["empty"]))
    with open(os.path.join(args.out_dir, "texture_mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
