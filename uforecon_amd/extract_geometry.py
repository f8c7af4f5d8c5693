"""Depth maps of the DTU test scans from their images: the `--extract_geometry` branch of the reference's main.py
(:145-163, 186-190, 229-230) under main.py's flag names, so that script/eval_dtu_*.sh's command line carries over.

    python -m uforecon_amd.extract_geometry --set 0 --volume_type correlation --depth_pos_encoding --mvs_depth_guide 1 \\
        --explicit_similarity --test_n_view 3 --test_ref_view 23 24 33 --test_dir DTU_TEST --load_ckpt uforecon.ckpt --out_dir OUT

For every scan and every render view: `dtu_scan.DtuScan` makes the batch, `pipeline.UFOReconInference.extract_geometry`
renders it and writes `<out_dir>/depth/<scan>/<%08d>.npy`, `<out_dir>/rgb/<scan>/<%08d>.jpg` and
`<out_dir>/<scan>/depth/<%08d>.png` (model.save_depth_outputs), the tree `python -m uforecon_amd.depth_fusion` and
`python -m uforecon_amd.tsdf` take as `--root_dir`.  The sampler's uniforms of a view come from a generator seeded by
(`--seed`, scan, view): a rerun writes the same files.

With `--test_general` (main.py:164-176) the scenes are `--test_scan` under `--test_dir`, read by `general_scan.GeneralScan`
(`--dataset blendedmvs | mvimage`, `--use_mask`); `--scans`, `--set` and `--original_img_wh` are not read, the image size is
the dataset's unless `--img_wh` is given, and the files are named `refview<i>` after each batch's reference view -- the tree
`python -m uforecon_amd.tsdf --dataset general --test_scan ...` reads.  A flag value the mirror does not implement (`--volume_type
featuregrid`, a missing `--explicit_similarity`, another cascade layout ...) ends the command with one line, exit code 2.
"""
from __future__ import annotations

import argparse
import os
import sys
import zlib

import torch

from ._lib import MAX_VIEWS
from .clean_mesh import SET1_VIEWS
from .dtu_eval import DTU_SCANS

# what pipeline.UFOReconInference implements: flag -> the one value it takes (every shipped script of the reference passes these)
IMPLEMENTED = {"volume_type": "correlation", "explicit_similarity": True, "depth_pos_encoding": True, "use_dir_srdf": False,
               "ndepths": "48,32,8", "depth_inter_r": "4,2,1", "cr_base_chs": "8,8,8"}
PRECISIONS = {"default": None, "fp32": 0, "16bit": 1}      # ops.PRECISION_FP32 / PRECISION_16BIT
IMG_MULTIPLE = 32     # the first cascade stage's volume is (H/4, W/4), and the 3-D U-Nets halve every extent three times (unet3d.py)


def make_parser():
    """main.py's testing flags with main.py's defaults, then this project's own."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--test_dir", dest="test_dir", type=str, help="directory of test dataset")
    parser.add_argument("--out_dir", dest="out_dir", type=str, help="directory of to save test result")
    parser.add_argument("--load_ckpt", dest="load_ckpt", type=str, default=False, help="load pretrained lightning ckpt")
    parser.add_argument("--extract_geometry", dest="extract_geometry", action="store_true", help="accepted: this command is that branch")
    parser.add_argument("--test_ray_num", dest="test_ray_num", type=int, default=1200, help="accepted and ignored: chunking is internal")
    parser.add_argument("--test_sample_coarse", dest="test_sample_coarse", type=int, default=64)
    parser.add_argument("--test_sample_fine", dest="test_sample_fine", type=int, default=64)
    parser.add_argument("--test_coarse_only", dest="test_coarse_only", action="store_true", help="only use coarse samples during testing")
    parser.add_argument("--test_n_view", dest="test_n_view", type=int, default=3)
    parser.add_argument("--test_ref_view", type=int, nargs="+", default=[23, 24, 33, 22, 15, 34, 14, 32, 16, 35, 25])
    parser.add_argument("--ndepths", type=str, default="48,32,8", help="ndepths")
    parser.add_argument("--depth_inter_r", type=str, default="4,2,1", help="depth_intervals_ratio")
    parser.add_argument("--cr_base_chs", type=str, default="8,8,8", help="cost regularization base channels")
    parser.add_argument("--view_selection_type", type=str, default="random", choices=["random", "best"], help="accepted and ignored")
    parser.add_argument("--mvs_depth_guide", type=int, default=0, help="use mvs depth map as guidance")
    parser.add_argument("--volume_type", type=str, default="correlation", choices=["featuregrid", "correlation"])
    parser.add_argument("--volume_reso", dest="volume_reso", type=int, default=96, help="accepted and ignored (featuregrid only)")
    parser.add_argument("--use_dir_srdf", action="store_true", help="use direction srdf")
    parser.add_argument("--depth_pos_encoding", action="store_true", help="use depth pos encoding")
    parser.add_argument("--explicit_similarity", action="store_true", help="use explicit similarity")
    parser.add_argument("--set", dest="set", type=int, default=0, help="two sets are provided by SparseNeuS")
    parser.add_argument("--test_general", dest="test_general", action="store_true", help="test on custom dataset")
    parser.add_argument("--test_scan", dest="test_scan", type=str, nargs="+",
                        default=["5aa235f64a17b335eeaf9609", "5ba19a8a360c7c30c1c169df", "5adc6bd52430a05ecb2ffb85", "5bf7d63575c26f32dbf7413b"])
    parser.add_argument("--dataset", dest="dataset", type=str, default="blendedmvs", help="dataset name")
    parser.add_argument("--use_mask", dest="use_mask", action="store_true", help="use mask")
    # ---- this project's own
    parser.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS, help="scan numbers (default: the reference's 15 test scans)")
    parser.add_argument("--img_wh", type=int, nargs=2, default=[800, 640], help="width and height the images are resized to")
    parser.add_argument("--original_img_wh", type=int, nargs=2, default=[1600, 1200], help="size the camera files' K refers to")
    parser.add_argument("--seed", type=int, default=0, help="seed of the samplers' uniforms")
    parser.add_argument("--precision", choices=sorted(PRECISIONS), default="default", help="matrix precision of the ray path")
    return parser


def unimplemented(args):
    """One line naming the first flag value outside what the mirror implements, or None."""
    for flag, want in IMPLEMENTED.items():
        if getattr(args, flag) != want:
            return f"--{flag} {getattr(args, flag)!r} is not implemented here (only {want!r}: what the reference's scripts pass)"
    if args.mvs_depth_guide <= 0:
        return "--mvs_depth_guide 0 is not implemented here (the ray path reads the MVS depth: pass --mvs_depth_guide 1)"
    if getattr(args, "test_general", False):
        # the custom-scene rule: a batch is the reference view plus the first test_n_view - 1 of --test_ref_view (a scene's
        # pair file is checked when the scene is opened)
        most = min(len(args.test_ref_view) + 1, MAX_VIEWS)
        if not 2 <= args.test_n_view <= most:
            return (f"--test_n_view {args.test_n_view} is not implemented here (2 .. {most}: the reference view and up to "
                    f"{len(args.test_ref_view)} of --test_ref_view)")
        from .general_scan import DATASET_WH

        if args.dataset not in DATASET_WH:
            return f"--dataset {args.dataset!r} is not implemented here (one of {sorted(DATASET_WH)})"
        return None
    views = args.test_ref_view if args.set == 0 else SET1_VIEWS
    if not 2 <= args.test_n_view <= min(len(views), MAX_VIEWS):
        return f"--test_n_view {args.test_n_view} is not implemented here (2 .. {min(len(views), MAX_VIEWS)} of the {len(views)} listed views)"
    return None


def parse_args(argv=None, parser=None):
    """`make_parser()`'s arguments with the two image sizes left open (None) unless given: `resolve_img_wh` fills them in."""
    parser = parser or make_parser()
    parser.set_defaults(img_wh=None, original_img_wh=None)
    return parser.parse_args(argv)


def resolve_img_wh(args):
    """(img_wh, original_img_wh) of a command line: what was given, else 800x640 of 1600x1200 for DTU and the dataset's own
    size for --test_general (which reads each picture's size from its file and ignores --original_img_wh)."""
    if args.test_general:
        from .general_scan import DATASET_WH

        default = list(DATASET_WH[args.dataset])
    else:
        default = [800, 640]
    return (list(args.img_wh) if args.img_wh is not None else default,
            list(args.original_img_wh) if args.original_img_wh is not None else [1600, 1200])


def scan_seed(scan_id: str) -> int:
    """what stands in `view_uniforms` for the scan number of a custom scene"""
    return zlib.crc32(str(scan_id).encode("utf-8"))


def view_uniforms(seed: int, scan: int, view: int, point_num: int, point_num_2: int, rays: int, coarse_only: bool = False):
    """(U1 (point_num, rays), U2 (point_num_2, rays) or None): the sampler uniforms of one render view, from their own generator"""
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(scan) * 1_009 + int(view)) % (2 ** 62))
    U1 = torch.rand(point_num, rays, generator=g)
    return U1, (None if coarse_only else torch.rand(point_num_2, rays, generator=g))


def load_checkpoint(net, path):
    """`torch.load(path)["state_dict"]` (a Lightning checkpoint) or a bare state dict, strict."""
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:  # noqa: BLE001 -- a Lightning file also pickles its hyper-parameters (an argparse.Namespace)
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    net.load_state_dict(ckpt["state_dict"] if "state_dict" in ckpt else ckpt, strict=True)


def load_net(args, dev):
    from .pipeline import UFOReconInference

    net = UFOReconInference(args)
    if args.load_ckpt:
        load_checkpoint(net, args.load_ckpt)
        print("Model loaded:", args.load_ckpt)
    else:
        print("no --load_ckpt: the model keeps its initial weights", file=sys.stderr)
    net = net.to(dev)
    net.precision = PRECISIONS[args.precision]
    return net


def main_general(parser, args):
    """The --test_general branch (main.py:164-176): one `GeneralScan` per --test_scan; --scans, --set and --original_img_wh are
    not read.  Every batch is named by its reference view: the files are `refview<i>.npy / .jpg / .png`, which is what
    `python -m uforecon_amd.tsdf --dataset general --test_scan ...` looks for."""
    from .general_scan import GeneralScan

    if args.img_wh[0] % IMG_MULTIPLE or args.img_wh[1] % IMG_MULTIPLE:
        parser.error(f"--img_wh {args.img_wh[0]} {args.img_wh[1]}: width and height must be multiples of {IMG_MULTIPLE} "
                     "(the first cascade stage works at a quarter of the size, and its U-Net halves that three times)")
    scenes = []
    for scan in args.test_scan:        # every scene is opened before the model is built: a missing file costs nothing
        try:
            scenes.append(GeneralScan(args.test_dir, scan, n_views=args.test_n_view, test_ref_view=args.test_ref_view, dataset=args.dataset,
                                      use_mask=args.use_mask, img_wh=args.img_wh, device="cuda:0"))
        except FileNotFoundError as e:
            parser.error(f"{scan}: {e.filename} is missing under --test_dir {args.test_dir}")
        except ValueError as e:
            parser.error(f"{scan}: --test_n_view {args.test_n_view}: {e}")
    net = load_net(args, torch.device("cuda:0"))
    for frames in scenes:
        for i in range(len(frames)):
            try:
                batch = frames[i]
            except FileNotFoundError as e:
                parser.error(f"{frames.scan_id}: {e.filename} is missing under --test_dir {args.test_dir}")
            ref_view = frames.metas[i][0]
            H, W = batch["source_imgs"].shape[-2:]
            U = view_uniforms(args.seed, scan_seed(frames.scan_id), ref_view, net.point_num, net.point_num_2, H * W, args.test_coarse_only)
            net.extract_geometry(batch, out_dir=args.out_dir, uniforms=U)
            print("%s reference view %d -> %s" % (frames.scan_id, ref_view, os.path.join(args.out_dir, "depth", frames.scan_id, "refview%d.npy" % ref_view)))
    return 0


def main(argv=None):
    from .dtu_scan import DtuScan

    parser = make_parser()
    args = parse_args(argv, parser)
    why = unimplemented(args)
    if why is None and not (args.test_dir and args.out_dir):
        why = "--test_dir and --out_dir are required"
    if why is not None:
        parser.error(why)
    args.img_wh, args.original_img_wh = resolve_img_wh(args)
    args.extract_geometry = True
    if args.test_general:
        return main_general(parser, args)
    dev = torch.device("cuda:0")
    net = load_net(args, dev)
    for scan in args.scans:
        try:
            frames = DtuScan(args.test_dir, "scan%d" % scan, n_views=args.test_n_view, img_wh=args.img_wh,
                             original_img_wh=args.original_img_wh, set=args.set, test_view_pair=args.test_ref_view, device=dev)
        except FileNotFoundError as e:
            parser.error(f"scan{scan}: {e.filename} is missing under --test_dir {args.test_dir}")
        for view, batch in enumerate(frames):
            H, W = batch["source_imgs"].shape[-2:]
            U = view_uniforms(args.seed, scan, view, net.point_num, net.point_num_2, H * W, args.test_coarse_only)
            net.extract_geometry(batch, out_dir=args.out_dir, uniforms=U)
            print("scan%d view %d -> %s" % (scan, view, os.path.join(args.out_dir, "depth", "scan%d" % scan, "%08d.npy" % view)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
