"""Training on the DTU training layout: the training branch of the reference's main.py (:112-143, 186-227: `trainer.fit` over
`UFORecon.training_step` / `configure_optimizers` with a `ModelCheckpoint` on val/loss_depth_fine), under main.py's flag names.

    python -m uforecon_amd.train --root_dir DTU_TRAINING --split_filepath lists/train.txt --val_split_filepath lists/test.txt \\
        --load_ckpt uforecon.ckpt --logdir OUT --batch_size 1 --max_epochs 16 --volume_type correlation --depth_pos_encoding \\
        --mvs_depth_guide 1 --explicit_similarity --train_n_view 4 --test_n_view 3 --test_ref_view 23 24 33 \\
        --view_selection_type best

An epoch is a permutation of the train items (`dtu_train.DtuTrain`, 'train' split) that depends on (`--seed`, epoch) alone; a step
is `pipeline.UFOReconTraining.training_step` -> `backward` -> `optim.Adam.step()` -> `zero_grad(set_to_none=True)`, one frame per
step, its rays and sampler uniforms from a device generator seeded by (`--seed`, global step): a rerun reproduces the run up to
the order in which the backward's scatter adds floats.  After every epoch the 'test' split with `--test_ref_view` is validated as
`uforecon_amd.validate` does, the epoch line is appended to `<logdir>/train_log.jsonl` (next to every `--log_every`-th step's), and
`<logdir>/checkpoints/epoch=NN.ckpt` is written with `torch.save`: `state_dict` (the reference's 530 keys), `epoch`,
`global_step`, `optimizer_states` = [torch.optim.Adam's format], `monitor` = {"val/loss_depth_fine": value}.  The 15 best files by
that score are kept (main.py:197-203), the rest deleted.  `--load_ckpt` loads weights only; `--resume` also restores the
optimizer, the epoch and the step.  Only `state_dict` is claimed to be what Lightning's loader reads.

The frozen TransMVSNet stays in eval mode while training (pipeline.UFOReconTraining): its BatchNorm statistics are the
checkpoint's before and after.  A flag value the mirror does not implement ends the command with one line, exit code 2.
"""
from __future__ import annotations

import json
import os
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import torch

from . import validate as V
from .extract_geometry import PRECISIONS, load_checkpoint

MONITOR = "val/loss_depth_fine"       # main.py:198
SAVE_TOP_K = 15                       # main.py:201
MAX_PREFETCH_THREADS = 4
MAX_RAYS = 4096                       # ufr_select_rays


def make_parser():
    """main.py's training flags with main.py's defaults (validate.make_parser's, + the ones only training reads), then this
    project's own."""
    parser = V.make_parser()
    parser.description = __doc__.split("\n")[0]
    for a in parser._actions:
        if a.dest == "train_ray_num":
            a.help = "ray number in one image"
        elif a.dest == "max_frames":
            a.help = "another name of --max_val_frames"
    parser.add_argument("--batch_size", dest="batch_size", type=int, default=2, help="batch size (only 1 is implemented)")
    parser.add_argument("--max_epochs", dest="max_epochs", type=int, default=16, help="max num of epochs")
    parser.add_argument("--uforecon_lr", dest="uforecon_lr", type=float, default=1.e-4, help="learning rate for uforecon")
    parser.add_argument("--weight_rgb", dest="weight_rgb", type=float, default=1.0)
    parser.add_argument("--weight_depth", dest="weight_depth", type=float, default=1.0)
    # ---- this project's own
    parser.add_argument("--val_split_filepath", type=str, default=None, help="the validation scans (default: the training scans)")
    parser.add_argument("--max_steps", type=int, default=0, help="stop after this many optimizer steps (0: no limit)")
    parser.add_argument("--max_val_frames", type=int, default=0, help="validate this many frames per epoch (0: all)")
    parser.add_argument("--train_items", type=int, nargs="+", default=None, help="an epoch is a permutation of these item indices only")
    parser.add_argument("--log_every", type=int, default=50, help="write every N-th step's losses to train_log.jsonl")
    parser.add_argument("--resume", type=str, default=None, help="a checkpoint of this command: weights, optimizer, epoch and step")
    parser.add_argument("--prefetch", type=int, default=2, help="decode the next N items' files on worker threads (0: none)")
    return parser


def unimplemented(args):
    """One line naming the first flag value outside what the mirror implements, or None."""
    if args.val_only:
        return "--val_only is not implemented here (validation alone is `python -m uforecon_amd.validate --val_only`)"
    if args.batch_size != 1:
        return f"--batch_size {args.batch_size} is not implemented here (one frame per step: pass --batch_size 1)"
    why = V.unimplemented(args)       # the flags of the ray path, and the source views of training and validation frames
    if why is not None:
        return why
    if not 1 <= args.train_ray_num <= MAX_RAYS:
        return f"--train_ray_num {args.train_ray_num} is not implemented here (the ray draw takes 1 .. {MAX_RAYS})"
    if args.prefetch < 0 or args.log_every < 1 or args.max_epochs < 0:
        return "--prefetch must be >= 0, --log_every >= 1 and --max_epochs >= 0"
    return None


def epoch_permutation(seed: int, epoch: int, items):
    """The order of ``items`` in epoch ``epoch``: a function of (seed, epoch) and the items alone."""
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(epoch) * 7919 + 17) % (2 ** 62))
    items = list(items)
    return [items[i] for i in torch.randperm(len(items), generator=g).tolist()]


def step_seed(seed: int, global_step: int) -> int:
    return (int(seed) * 1_000_003 + int(global_step) * 104_729 + 29) % (2 ** 62)


class TopK:
    """ModelCheckpoint(save_top_k=k, mode='min') on files: `add` records a written file with its score and deletes whatever
    fell out of the k best (on equal scores the older file stays)."""

    def __init__(self, k: int = SAVE_TOP_K, kept=None):
        self.k = int(k)
        self.kept = [(float(s), str(p)) for s, p in (kept or [])]       # in the order written

    def wants(self, score: float) -> bool:
        return len(self.kept) < self.k or float(score) < max(s for s, _ in self.kept)

    def add(self, path: str, score: float):
        self.kept.append((float(score), str(path)))
        removed = []
        while len(self.kept) > self.k:
            worst = max(range(len(self.kept)), key=lambda i: (self.kept[i][0], i))     # the largest score, the newest among equals
            removed.append(self.kept.pop(worst)[1])
        for p in removed:
            if os.path.exists(p):
                os.remove(p)
        return removed


def save_checkpoint(path, net, optimizer, epoch: int, global_step: int, score: float, kept=()):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in net.state_dict().items()}, "epoch": int(epoch),
                "global_step": int(global_step), "optimizer_states": [optimizer.state_dict()],
                "monitor": {MONITOR: float(score)}, "kept_checkpoints": [[s, os.path.basename(p)] for s, p in kept]}, path)


class Prefetch:
    """``ds[i]`` for i in ``order``, with the files of the next ``ahead`` items decoded on worker threads (at most 4) while the
    caller works on the current one.  ``ds`` splits an item into `load(i)` (host-only file decoding, safe on any thread) and
    `finish(i, loaded)` (the rest, run here on the caller's thread), with ``ds[i] == ds.finish(i, ds.load(i))``: the batches
    and their order are those of the plain loop.  A worker's exception is raised where its item is consumed."""

    def __init__(self, ds, order, ahead: int = 2):
        self.ds, self.order, self.ahead = ds, list(order), max(0, int(ahead))

    def __iter__(self):
        if self.ahead == 0:
            for i in self.order:
                yield i, self.ds[i]
            return
        pool = ThreadPoolExecutor(max_workers=min(MAX_PREFETCH_THREADS, self.ahead))
        try:
            pending, nxt = deque(), 0
            for pos, i in enumerate(self.order):
                while nxt < len(self.order) and nxt <= pos + self.ahead:
                    pending.append(pool.submit(self.ds.load, self.order[nxt]))
                    nxt += 1
                loaded = pending.popleft().result()
                yield i, self.ds.finish(i, loaded)
        finally:
            pool.shutdown(wait=True, cancel_futures=True)


def main(argv=None):
    fit(argv)
    return 0


def fit(argv=None):
    """The command.  Returns what it ends with -- dict(net, optimizer, epoch (the next one), global_step) -- for callers that go on
    from there (tests)."""
    from .dtu_train import DtuTrain
    from .pipeline import UFOReconTraining

    parser = make_parser()
    args = parser.parse_args(argv)
    why = unimplemented(args)
    if why is None and not args.root_dir:
        why = "--root_dir is required"
    if why is None and not (args.split_filepath or args.scans):
        why = "--split_filepath or --scans is required"
    if why is not None:
        parser.error(why)
    args.extract_geometry = False
    args.max_val_frames = args.max_val_frames or args.max_frames
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)          # the initial weights of a run without --load_ckpt (main.py: seed_everything(0))
    net = UFOReconTraining(args)
    start_epoch, global_step, resumed = 0, 0, None
    if args.resume:
        resumed = torch.load(args.resume, map_location="cpu", weights_only=True)
        net.load_state_dict(resumed["state_dict"], strict=True)
        start_epoch, global_step = int(resumed["epoch"]) + 1, int(resumed["global_step"])
        print(f"Resumed: {args.resume} (epoch {start_epoch}, global_step {global_step})")
    elif args.load_ckpt:
        load_checkpoint(net, args.load_ckpt)
        print("Model loaded:", args.load_ckpt)
    else:
        print("no --load_ckpt: the model keeps its initial weights", file=sys.stderr)
    net = net.to(dev)
    net.precision = PRECISIONS[args.precision]
    opt = net.configure_optimizers()
    ckpt_dir = os.path.join(args.logdir, "checkpoints")
    keeper = TopK(SAVE_TOP_K)
    if resumed is not None:
        opt.load_state_dict(resumed["optimizer_states"][0])
        keeper = TopK(SAVE_TOP_K, [(s, os.path.join(ckpt_dir, name)) for s, name in resumed.get("kept_checkpoints", [])])
    try:
        ds = DtuTrain(args.root_dir, "train", n_views=args.train_n_view, split_filepath=args.split_filepath, scans=args.scans,
                      pair_filepath=args.pair_filepath, view_selection_type=args.view_selection_type, device=dev, seed=args.seed)
        val_scans = None if args.val_split_filepath else args.scans
        ds_val = DtuTrain(args.root_dir, "test", n_views=args.test_n_view, split_filepath=args.val_split_filepath or args.split_filepath,
                          scans=val_scans, pair_filepath=args.pair_filepath, test_ref_views=args.test_ref_view,
                          view_selection_type=args.view_selection_type, device=dev, seed=args.seed)
    except FileNotFoundError as e:
        parser.error(f"{e.filename} is missing (--root_dir {args.root_dir})")
    items = list(range(len(ds))) if args.train_items is None else list(args.train_items)
    if not items or min(items) < 0 or max(items) >= len(ds):
        parser.error(f"--train_items must lie in 0 .. {len(ds) - 1} (the split has {len(ds)} items)")
    print("dtu_dataset_train:", len(ds))
    print("dtu_dataset_val:", len(ds_val))
    os.makedirs(args.logdir, exist_ok=True)
    log = open(os.path.join(args.logdir, "train_log.jsonl"), "a")

    def record(**kw):
        log.write(json.dumps(kw) + "\n")
        log.flush()

    if resumed is not None:
        record(kind="resume", epoch=start_epoch, global_step=global_step, checkpoint=args.resume)
    gen = torch.Generator(device=dev)
    done = False
    epoch = start_epoch - 1
    for epoch in range(start_epoch, args.max_epochs):
        net.train()
        try:
            for i, batch in Prefetch(ds, epoch_permutation(args.seed, epoch, items), args.prefetch):
                gen.manual_seed(step_seed(args.seed, global_step))
                loss, logs = net.training_step(batch, global_step, generator=gen)
                loss.backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
                global_step += 1
                if global_step % args.log_every == 0:        # (the one place a step waits for the device)
                    vals = {k: float(v) for k, v in logs.items()}
                    record(kind="step", epoch=epoch, global_step=global_step, item=i, meta=batch["meta"][0], **vals)
                    print("epoch %d step %d %s loss %.6f" % (epoch, global_step, batch["meta"][0], vals["train/loss_all"]))
                if args.max_steps > 0 and global_step >= args.max_steps:
                    done = True
                    break
        except FileNotFoundError as e:
            parser.error(f"{e.filename} is missing (--root_dir {args.root_dir})")
        net.eval()
        parts = V.validate_frames(net, ds_val, args, args.max_val_frames, parser)
        if not parts:
            parser.error("no validation frames: the split and --test_ref_view select nothing")
        end = dict(net.validation_epoch_end(parts), frames=len(parts))
        score = end[MONITOR]
        path = os.path.join(ckpt_dir, "epoch=%02d.ckpt" % epoch)
        saved = keeper.wants(score)
        if saved:
            save_checkpoint(path, net, opt, epoch, global_step, score, keeper.kept + [(score, path)])
            keeper.add(path, score)
        record(kind="epoch", epoch=epoch, global_step=global_step, checkpoint=path if saved else None, **end)
        print(json.dumps(dict(end, epoch=epoch, global_step=global_step)))
        if done:
            break
    log.close()
    print("end")
    return dict(net=net, optimizer=opt, epoch=epoch + 1, global_step=global_step)


if __name__ == "__main__":
    sys.exit(main())
