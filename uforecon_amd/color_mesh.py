"""Mesh colouring on the GPU: per-vertex colour from the photographs, visibility-aware -- the stage between ``clean_mesh`` and
``render_trajectory --color vertex`` that the reference does not have.  Its hot loop is a HIP kernel (csrc/mesh_color.hip
through ``ops.mesh_vertex_colors`` and ``ops.mesh_color_fill``); include/ufr.h states every rule, tests/color_mesh_ref.py
restates them in numpy.

    python -m uforecon_amd.color_mesh --mesh_dir OUT/mesh/final --root_dir DTU_TEST --out_dir OUT/mesh/color
        [--views 23 24 33 ... | --all_views] [--scans ...] [--ply FILE ...] [--mode mean|best] [--depth_tol T] [--min_cos C]
        [--power P] [--fill_rounds R] [--fill_color r g b] [--no_occlusion]

reads ``<mesh_dir>/scan<N>.ply``, ``<root_dir>/cameras/{:0>8}_cam.txt`` and ``<root_dir>/scan<N>/image/{:0>6}.png`` (the names
``clean_mesh`` and ``dtu_scan`` use), writes ``<out_dir>/scan<N>.ply`` with red / green / blue per vertex and
``<out_dir>/color_mesh.json`` with the counts and the milliseconds of every stage.  ``--ply`` colours the named mesh files
instead, paired in order with ``--scans`` (whose pictures they take), each to ``<out_dir>/<file stem>.ply``.

1. area-weighted vertex normals (``ops.raster_vertex_normals``);
2. per view the mesh's own z-depth at the picture's size (``ops.raster_frames(return_depth=True)``, one call per view);
3. every vertex is projected into every view in fp64, tested against that view's depth map (all four texels of its bilinear
   footprint must show a hit that is not nearer than the vertex), against the viewing angle, and sampled bilinearly;
4. the views are blended with weights cos^power (``mean``) or the most frontal one is taken (``best``);
5. vertices that no view saw take the mean of their coloured neighbours, one edge further per round (``fill_rounds``).

The defaults are derived, not tuned on a real scan (DESIGN.md 3.4.13 gives the derivations); no real scan has been coloured.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

from .clean_mesh import TEST_REF_VIEW, ray_camera, read_cam_file
from .dtu_eval import DTU_SCANS, read_ply

ALL_VIEWS = list(range(49))                      # the 49 photographs of a DTU scan
DEPTH_TOL = 0.005                                # 3 mm at 600 mm: 2.5 pixels of an 80-degree slope (1.2 mm a pixel)
MIN_COS = 0.2                                    # a 0.2 mm pixel smears over 1 mm of surface: about one mesh edge
POWER = 2                                        # a pose error moves the sample by 1 / cos: inverse variance = cos^2
FILL_ROUNDS = 8                                  # the rim the conservative tests leave is a few edges wide; 8 rounds close 16
FILL_COLOR = (128, 128, 128)
STATE_EMPTY, STATE_SEEN, STATE_FILLED = 0, 1, 2  # the values of the state array


def projection_camera(K, E):
    """(k 3x3, w2c 4x4, centre 3) float64 of one ``(K, E)`` pair as in a ``*_cam.txt``: k = K / K[2,2], w2c = E / E[3,3] (1
    unless E was scaled as a whole), centre = inv(w2c)[:3,3] -- the fp64 side of the camera ``clean_mesh.ray_camera`` narrows
    to float32 for the depth maps."""
    K64 = np.asarray(K, np.float32).astype(np.float64)
    E64 = np.asarray(E, np.float32).astype(np.float64)
    w2c = E64 / E64[3, 3]
    return K64 / K64[2, 2], w2c, np.linalg.inv(w2c)[:3, 3].copy()


def color_mesh(verts, faces, cams, images, mode="mean", depth_tol=DEPTH_TOL, min_cos=MIN_COS, power=POWER, fill_rounds=FILL_ROUNDS,
               fill_color=FILL_COLOR, occlusion=True, z_min=0.0, return_timings=False, device="cuda"):
    """Vertex colours of a mesh from photographs, in memory.  ``verts`` (V,3) any float dtype (widened to float64 once),
    ``faces`` (F,3) integers; ``cams``: one ``(K 3x3, E 4x4)`` pair per view as ``clean_mesh.read_cam_file`` returns them;
    ``images``: one (H,W,3) uint8 picture per view, all of one size, at most 64.  Returns ``colors`` (V,3) uint8, ``views_used``
    (V,) uint8 and ``state`` (V,) uint8 (``STATE_SEEN``: coloured by a view, ``STATE_FILLED``: by its neighbours,
    ``STATE_EMPTY``: ``fill_color``) as numpy arrays; with ``return_timings`` also a dict of milliseconds per stage.

    The views are not processed in groups: the colour kernel takes all views of the call, so a vertex's sum runs over them in
    ascending order inside one thread and there is no grouping that could change a bit.  What is resident is one (n,H,W,3)
    uint8 and one (n,H,W) float32 tensor -- 13.4 MB a view at 1200 x 1600, 0.66 GB for all 49.  Only the depth maps are made
    view by view (``k_inv`` is shared within a call of ``ops.raster_frames``), each into its own slice."""
    import torch

    from . import ops
    from ._lib import UfrError

    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    cams, images = list(cams), [np.asarray(m) for m in images]
    if len(cams) != len(images) or not cams:
        raise UfrError(f"color_mesh: {len(cams)} cameras, {len(images)} pictures (need one picture per camera, at least one)")
    if len(cams) > ops.MESH_MAX_VIEWS:
        raise UfrError(f"color_mesh: {len(cams)} views (at most {ops.MESH_MAX_VIEWS})")
    for m in images:
        if m.ndim != 3 or m.shape[2] != 3 or m.dtype != np.uint8 or m.shape != images[0].shape:
            raise UfrError(f"color_mesh: pictures must be (H, W, 3) uint8 of one size, got {[(x.shape, str(x.dtype)) for x in images]}")
    V, F = len(verts), len(faces)
    if F == 0 or V == 0:
        raise UfrError(f"color_mesh: the mesh has {V} vertices and {F} faces (need at least one face)")
    if faces.min() < 0 or faces.max() >= V:                        # the one index check: every call below trusts it
        raise UfrError(f"color_mesh: face indices span {faces.min()}..{faces.max()}, the mesh has {V} vertices")
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
    tn = ops.raster_vertex_normals(tv, tf)
    tock("normals_ms")
    tick()
    depth = None
    if occlusion:
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        for i, (K, E) in enumerate(cams):
            k_inv, c2w = ray_camera(K, E)
            depth[i] = ops.raster_frames(tv, tf, k_inv, c2w[None], H, W, return_depth=True, check_indices=False)["depth"][0]
    tock("depth_ms")
    tick()
    pk, pw, pc = (np.stack(a) for a in zip(*[projection_camera(K, E) for K, E in cams]))
    colors, used = ops.mesh_vertex_colors(tv, tn, ti, depth, pk, pw, pc, z_min=z_min, depth_tol=depth_tol, min_cos=min_cos,
                                          power=power, mode=mode, fill=fill_color)
    tock("color_ms")
    tick()
    colors, has, rounds_run = ops.mesh_color_fill(tf, colors, used, fill_rounds)
    tock("fill_ms")
    used = used.cpu().numpy()
    state = np.where(used > 0, STATE_SEEN, np.where(has.cpu().numpy() != 0, STATE_FILLED, STATE_EMPTY)).astype(np.uint8)
    ms["fill_rounds_run"] = rounds_run
    out = (colors.cpu().numpy(), used, state)
    return out + (ms,) if return_timings else out


def write_ply(filename, verts, faces, colors, normals=None):
    """binary little-endian PLY: float x / y / z, (float nx / ny / nz,) uchar red / green / blue, ``list uchar int`` faces --
    what ``dtu_eval.read_ply(with_colors=True)`` reads back bit for bit and ``render_trajectory --color vertex`` draws"""
    verts = np.asarray(verts).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    colors = np.asarray(colors)
    if colors.shape != verts.shape or colors.dtype != np.uint8:
        raise ValueError(f"write_ply: colors {colors.shape} {colors.dtype}: expected {verts.shape} uint8")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        normals = np.asarray(normals).reshape(-1, 3)
        if normals.shape != verts.shape:
            raise ValueError(f"write_ply: normals {normals.shape}: expected {verts.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(len(verts), dtype=fields)
    for j, a in enumerate("xyz"):
        vrec[a] = verts[:, j]
        if normals is not None:
            vrec["n" + a] = normals[:, j]
    for j, a in enumerate(("red", "green", "blue")):
        vrec[a] = colors[:, j]
    frec = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = faces
    props = "".join("property %s %s\n" % ("uchar" if t == "u1" else "float", name) for name, t in fields)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\nproperty list uchar int vertex_indices\n"
              "end_header\n" % (len(vrec), props, len(frec)))
    with open(filename, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_image(filename):
    """(H,W,3) uint8 RGB"""
    from PIL import Image

    return np.ascontiguousarray(np.array(Image.open(filename).convert("RGB"), dtype=np.uint8))


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh_dir", type=str, default="./outputs/mesh/final", help="directory of scan<N>.ply")
    parser.add_argument("--root_dir", type=str, default="./dtu_test", help="dataset (cameras/<view>_cam.txt, scan<N>/image/<view>.png)")
    parser.add_argument("--out_dir", type=str, default="./outputs/mesh/color", help="scan<N>.ply and color_mesh.json go here")
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the 15 DTU test scans)")
    group = parser.add_mutually_exclusive_group()
    group.add_argument("--views", type=int, nargs="+", default=TEST_REF_VIEW, help="the photographs to colour from")
    group.add_argument("--all_views", action="store_true", help="all 49 photographs of a DTU scan")
    parser.add_argument("--ply", type=str, nargs="+", default=None,
                        help="colour these mesh files instead of scan<N>.ply, paired in order with --scans, each to <out_dir>/<file stem>.ply")
    parser.add_argument("--mode", choices=["mean", "best"], default="mean", help="blend the views by cos^power, or take the most frontal")
    parser.add_argument("--depth_tol", type=float, default=DEPTH_TOL, help="relative depth slack of the occlusion test")
    parser.add_argument("--min_cos", type=float, default=MIN_COS, help="views at a flatter angle than this cosine are not used")
    parser.add_argument("--power", type=int, default=POWER, help="weight of a view: cos^power (0 .. 8)")
    parser.add_argument("--fill_rounds", type=int, default=FILL_ROUNDS, help="neighbour-fill rounds for vertices no view saw")
    parser.add_argument("--fill_color", type=int, nargs=3, default=list(FILL_COLOR), help="colour of the vertices left empty")
    parser.add_argument("--no_occlusion", action="store_true", help="skip the depth maps: every view that contains a vertex colours it")
    return parser


def color_scan(mesh_path, root_dir, scan, views, out_path, **kw):
    """One scan: colours ``mesh_path`` from the pictures ``views`` of ``scan`` and writes ``out_path``.  Returns the report
    dict of ``color_mesh.json``.  Raises ValueError with one line for a missing picture or camera, pictures of unequal size and
    a mesh without faces."""
    verts, faces = read_ply(mesh_path)
    if faces is None or len(faces) == 0:
        raise ValueError(f"{mesh_path} has no faces")
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
    colors, used, state, ms = color_mesh(verts, faces, cams, images, return_timings=True, **kw)
    write_ply(out_path, verts, faces, colors)
    return dict(mesh=mesh_path, views=[int(v) for v in views], vertices=int(len(verts)), seen=int((state == STATE_SEEN).sum()),
                filled=int((state == STATE_FILLED).sum()), empty=int((state == STATE_EMPTY).sum()),
                views_used_histogram=np.bincount(used, minlength=len(views) + 1).tolist(), **ms)


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
            report[name] = color_scan(path, args.root_dir, scan, views, os.path.join(args.out_dir, name + ".ply"), mode=args.mode,
                                      depth_tol=args.depth_tol, min_cos=args.min_cos, power=args.power,
                                      fill_rounds=args.fill_rounds, fill_color=tuple(args.fill_color),
                                      occlusion=not args.no_occlusion)
        except ValueError as e:
            print("%s: %s" % (name, e))
            continue
        r = report[name]
        print("%s: %d vertices, %d seen, %d filled, %d left empty" % (name, r["vertices"], r["seen"], r["filled"], r["empty"]))
    with open(os.path.join(args.out_dir, "color_mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
