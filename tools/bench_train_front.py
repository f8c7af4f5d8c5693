"""Benchmark of the training front door: one full step of `pipeline.UFOReconTraining` -- frozen encode, the three frustums with
gradients, the ray draw, infer, loss, backward, optimizer -- on a synthetic train-layout frame at 512x640, 3 source views,
1024 rays, 64 + 64 samples, and each new piece against the torch forms it replaces, in the same process:
  (a) `optim.Adam.step()` against `torch.optim.Adam` in its default, `foreach=True` and `fused=True` forms, all on the gradients of
      that step (wall time of `--opt_iters` steps ending in a synchronise, the forms alternating, best of `--reps` rounds);
  (b) `ops.select_rays` against `argsort(u)[:k]` and `topk(k, largest=False)` on the GPU, n = 512 * 640, k = 1024 (same timing);
  (c) a step that reads its frame from disk (the synthetic tree of tests/dtu_train_golden.py, train items 7 and 275 in turn,
      PNG and PFM decoding included) with `train.Prefetch` on and off (wall time per step over `--disk_steps` steps).
Prints one JSON object; --out writes it to a file.  The parent of this tool has no front-door step: there is no "before" leg."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dtu_train_golden as G  # noqa: E402
from helpers import load_weights  # noqa: E402
from uforecon_amd import ops, optim, pipeline  # noqa: E402
from uforecon_amd import train as T  # noqa: E402
from uforecon_amd.scene import fill_state_dict, make_frame  # noqa: E402

DEV = "cuda:0"
H, W, NV, RAYS = 512, 640, 3, 1024


def _args():
    return argparse.Namespace(extract_geometry=False, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64, fine_sample=64,
                              volume_type="correlation", volume_reso=96, mvs_depth_guide=1, depth_pos_encoding=True,
                              use_dir_srdf=False, explicit_similarity=True, test_coarse_only=False, train_ray_num=RAYS,
                              test_n_view=NV, train_n_view=NV + 1, logdir=None, uforecon_lr=1e-4, weight_rgb=1.0, weight_depth=1.0)


def synthetic_batch(seed=0):
    """a train-layout frame of uforecon_amd.scene with what the encoder half reads added (as tests/test_gpu_validation_step.py)"""
    batch = make_frame(H, W, NV, seed=seed, train_layout=True).to(DEV).batch
    pm = {}
    for st, s in (("stage1", 4), ("stage2", 2), ("stage3", 1)):
        p = torch.zeros(1, NV, 2, 4, 4, device=DEV)
        p[0, :, 0] = batch["w2cs"][0, 1:]
        K = batch["intrinsics"][0, 1:].clone()
        K[:, :2] = K[:, :2] / s
        p[0, :, 1, :3, :3] = K
        p[0, :, 1, 3, 3] = 1.0
        pm[st] = p
    batch["proj_matrices"] = pm
    near, far = float(batch["near_fars"][0, 0, 0]), float(batch["near_fars"][0, 0, 1])
    batch["depth_values_org_scale"] = torch.linspace(near, far, 48, device=DEV)[None]
    batch["meta"] = ["synthetic"]
    return batch


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(legs, iters, reps):
    """{name: best ms per call} of the legs run in turn, `reps` rounds (+ one warm-up round)"""
    best = {k: float("inf") for k in legs}
    for r in range(reps + 1):
        for k, fn in legs.items():
            ms = wall_ms(fn, iters if r else max(3, iters // 10))
            if r:
                best[k] = min(best[k], ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--opt_iters", type=int, default=200)
    ap.add_argument("--disk_steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="write the result as JSON here")
    a = ap.parse_args()
    res = dict(image=f"{H}x{W}", source_views=NV, rays=RAYS, samples="64+64", device=torch.cuda.get_device_name(0))

    net = fill_state_dict(pipeline.UFOReconTraining(_args()), 21)
    net.load_state_dict(load_weights(), strict=False)
    net = net.to(DEV).train()
    opt = net.configure_optimizers()
    batch = synthetic_batch()
    gen = torch.Generator(device=DEV).manual_seed(1)

    def step(b=batch, keep_grads=False):
        loss, _ = net.training_step(b, 0, generator=gen)
        loss.backward()
        opt.step()
        if not keep_grads:
            opt.zero_grad(set_to_none=True)
        return loss

    for _ in range(a.warmup):
        step()
    res["front_door_step_ms"] = wall_ms(step, a.steps)
    res["front_door_step"] = (f"wall time per step over {a.steps} steps after {a.warmup} warm-up steps, frame resident on the device: frozen "
                              "encode + frustums with grad + ray draw + infer + loss + backward + optim.Adam")

    # ---- (a) the optimizer forms on the same gradients
    step(keep_grads=True)
    with_grad = [p for p in opt.param_groups[0]["params"] if p.grad is not None]
    grads = [p.grad.detach() for p in with_grad]
    forms = {"optim.Adam (ufr_adam_step)": lambda ps: optim.Adam(ps, lr=1e-4),
             "torch.optim.Adam (default)": lambda ps: torch.optim.Adam(ps, lr=1e-4),
             "torch.optim.Adam (foreach=True)": lambda ps: torch.optim.Adam(ps, lr=1e-4, foreach=True),
             "torch.optim.Adam (fused=True)": lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True)}
    legs = {}
    for name, make in forms.items():
        ps = [p.detach().clone().requires_grad_(True) for p in with_grad]
        for p, g in zip(ps, grads):
            p.grad = g                    # the step's own gradient tensors (cost_reg_2's: slices of one flat buffer)
        legs[name] = make(ps).step
    res["adam_step_ms"] = alternate(legs, a.opt_iters, a.reps)
    res["adam_tensors"], res["adam_floats"] = len(with_grad), sum(p.numel() for p in with_grad)
    opt.zero_grad(set_to_none=True)

    # ---- (b) the ray draw
    u = torch.rand(H * W, device=DEV, generator=gen)
    res["ray_draw_ms"] = alternate({"ops.select_rays": lambda: ops.select_rays(u, RAYS),
                                    "argsort(u)[:k]": lambda: torch.argsort(u)[:RAYS],
                                    "topk(k, largest=False)": lambda: u.topk(RAYS, largest=False, sorted=True).indices},
                                   a.opt_iters, a.reps)
    res["ray_draw"] = f"n = {H * W}, k = {RAYS}"

    # ---- (c) steps that read their frames from disk, prefetch on / off
    with tempfile.TemporaryDirectory() as tmp:
        root = G.write_tree(tmp)
        from uforecon_amd.dtu_train import DtuTrain

        ds = DtuTrain(root, "train", n_views=NV + 1, split_filepath=os.path.join(root, "scans.txt"), view_selection_type="best", device=DEV)
        order = [7, 275] * (a.disk_steps // 2)
        out = {}
        for r in range(a.reps + 1):
            for name, ahead in (("prefetch 0", 0), ("prefetch 2", 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _, b in T.Prefetch(ds, order, ahead):
                    step(b)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / len(order)
                if r:
                    out[name] = min(out.get(name, float("inf")), ms)
        res["disk_step_ms"] = out
        res["disk_step"] = f"wall time per step over {len(order)} steps, items 7 and 275 in turn, files decoded every step; best of {a.reps} rounds"
    res["timing"] = (f"adam_step_ms / ray_draw_ms: wall time per call over {a.opt_iters} calls ending in a synchronise, legs alternating, best of "
                     f"{a.reps} rounds after a warm-up round")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
