"""The training front door on the GPU: ufr_adam_step and ufr_select_rays against their torch statements, UFOReconTraining's
training_step against the pieces it is made of, our optimizer against torch's over a few steps, and the train command end to
end on the synthetic tree of tests/dtu_train_golden.py."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import dtu_train_golden as G
import train_front_ref as R
from helpers import load_weights
from uforecon_amd import ops, optim, pipeline
from uforecon_amd import train as T
from uforecon_amd._lib import UfrError
from uforecon_amd.extract_geometry import load_checkpoint
from uforecon_amd.scene import fill_state_dict, make_frame, sampler_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-3


# ------------------------------------------------------------------------------------------------------ ufr_adam_step
def _offset_view(offset):
    """a copy of t that starts `offset` floats into a larger buffer: 4-byte aligned only when `offset` is odd"""
    def place(i, t):
        buf = torch.zeros(t.numel() + offset(i), dtype=t.dtype, device=t.device)
        v = buf[offset(i):]
        v.copy_(t)
        return v
    return place


def _check(got, want, bounds, label):
    worst = 0.0
    for i, (g, w, b) in enumerate(zip(got, want, bounds)):
        err = float((g - w).abs().max())
        worst = max(worst, err / b)
        assert err <= b, (label, i, w.numel(), err, b)
    print(f"{label}: worst error / bound {worst:.3f} over {len(got)} tensors; "
          f"errors {[float('%.2e' % float((g - w).abs().max())) for g, w in zip(got, want)]}")


@pytest.mark.parametrize("layout", ["slices", "aligned"])
def test_adam_step_follows_torch_in_float64(layout):
    """5 steps on tensors of every size class (one lane, a part wave, around a wave, around a block's 16-byte part, more than
    one chunk).  `slices`: every gradient a slice of one buffer at an odd float offset, as CostRegNetWeightFn.backward hands
    them out, and parameter 3 a view at a non-zero offset -- 4-byte alignment only, the one-element path; `aligned`: fresh
    allocations, the 16-byte path with its tails.  Same yardstick and bound as the CPU test."""
    numels = (1, 3, 63, 64, 65, 255, 1328, 4097)
    params, grads = R.adam_case(numels, seed=1, skip=(5, 2))
    want, bounds = R.adam_bounds(params, grads, LR)
    kw = {}
    if layout == "slices":
        kw = dict(place=lambda i, t: _offset_view(lambda j: 3)(i, t) if i == 3 else t, place_grad=_offset_view(lambda j: 2 * j + 1))
        probe = kw["place_grad"](2, torch.zeros(5, device=DEV))
        assert probe.data_ptr() % 16 != 0 and probe.data_ptr() % 4 == 0
    got, opt = R.run_adam(lambda ps: optim.Adam(ps, lr=LR), params, grads, device=DEV, **kw)
    _check(got, want, bounds, f"ufr_adam_step ({layout})")
    ps = opt.param_groups[0]["params"]
    assert [float(opt.state[p]["step"]) for p in ps[:8]] == [5.0] * 5 + [4.0] + [5.0] * 2 and ps[8] not in opt.state
    assert torch.equal(got[8], params[8].double())


def test_adam_step_crosses_the_launch_split_and_keeps_zero_gradients_still():
    cap = ops.adam_table_capacity()
    numels = tuple(1 + (7 * i) % 13 for i in range(cap + 1))
    params, grads = R.adam_case(numels, seed=2, skip=(cap, 1), never=False)
    want, bounds = R.adam_bounds(params, grads, LR)
    got, _ = R.run_adam(lambda ps: optim.Adam(ps, lr=LR), params, grads, device=DEV)
    _check(got, want, bounds, f"ufr_adam_step ({cap + 1} tensors: two launches)")
    p = torch.randn(1000, device=DEV).requires_grad_(True)
    before = p.detach().clone()
    opt = optim.Adam([p], lr=LR)
    for _ in range(2):
        p.grad = torch.zeros_like(p)
        opt.step()
    assert torch.equal(p.detach(), before)


# ----------------------------------------------------------------------------------------------------- ufr_select_rays
def _inputs(n, kind):
    if kind == "rand":
        return torch.rand(n, generator=torch.Generator().manual_seed(n))
    if kind == "ties":
        return R.quantised_uniforms(n, seed=n)
    return torch.full((n,), 0.375)


@pytest.mark.parametrize("n,k", [(2048, 1024), (1961, 7), (64, 64), (1, 1), (327680, 1024), (5000, 4096)])
def test_select_rays_is_the_stable_argsort(n, k):
    for kind in ("rand", "ties", "equal"):
        u = _inputs(n, kind)
        got = ops.select_rays(u.to(DEV), k)
        assert got.dtype == torch.int64 and got.shape == (k,)
        assert torch.equal(got.cpu(), R.stable_first_k(u, k)), (n, k, kind)
        assert torch.equal(ops.select_rays(u.to(DEV), k), got)                 # a rerun: the same bits
        if kind == "equal":
            assert torch.equal(got.cpu(), torch.arange(k))


def test_select_rays_on_any_bit_pattern_gives_distinct_indices_in_range():
    n, k = 20000, 4096
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.int64)
    bits[::97] = 0x7FC00000                           # NaNs, infinities, negative zeros among them
    bits[1::97] = -0x00800000
    bits[2::97] = -0x80000000
    u = bits.to(torch.int32).view(torch.float32)
    got = ops.select_rays(u.to(DEV), k).cpu()
    assert got.shape == (k,) and int(got.min()) >= 0 and int(got.max()) < n and got.unique().numel() == k
    keys = bits & 0xFFFFFFFF                          # the patterns as unsigned integers: the order the header states
    assert torch.equal(got, torch.sort(keys, stable=True).indices[:k])


def test_select_rays_refuses_more_than_4096():
    with pytest.raises(UfrError, match="k=4097"):
        ops.select_rays(torch.rand(5000, device=DEV), 4097)
    with pytest.raises(UfrError):
        ops.select_rays(torch.rand(16, device=DEV), 17)


# ------------------------------------------------------------------------------------------------------- training_step
H, W, NV, RN = 32, 64, 3, 256


def _args(lr=1e-4):
    return argparse.Namespace(extract_geometry=False, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64,
                              fine_sample=64, volume_type="correlation", volume_reso=96, mvs_depth_guide=1,
                              depth_pos_encoding=True, use_dir_srdf=False, explicit_similarity=True, test_coarse_only=False,
                              train_ray_num=1024, test_n_view=NV, train_n_view=NV + 1, logdir=None, uforecon_lr=lr,
                              weight_rgb=1.0, weight_depth=1.0)


def _batch(seed=0):
    """tests/test_gpu_validation_step.py::_batch: a train-layout batch (dtu_train.py:442-495) plus what the encoder half reads."""
    fr = make_frame(H, W, NV, seed=seed, train_layout=True).to(DEV)
    batch = fr.batch
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
    batch["scale_mat"] = torch.diag(torch.tensor([1.5, 1.5, 1.5, 1.0], device=DEV))[None]
    batch["meta"] = ["scan24_light3_refview23"]
    gt = batch["depths_h"][0, 0]
    gt[::5, ::3] = 0.0
    gt[1, :] = far + 0.5
    return batch


@pytest.fixture(scope="module")
def initial_state():
    """the seeded weights every model of this file starts from: random encoder (seed 21) + the parity fixtures' ray path"""
    n = fill_state_dict(pipeline.UFOReconTraining(_args(), tune_convolutions=False), 21)
    n.load_state_dict(load_weights(), strict=False)
    return {k: v.clone() for k, v in n.state_dict().items()}


def _model(state, lr=1e-4):
    n = pipeline.UFOReconTraining(_args(lr), tune_convolutions=False)
    n.load_state_dict(state, strict=True)
    return n.to(DEV).train()


@pytest.fixture(scope="module")
def rays():
    idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))[:RN].sort().values[None].to(DEV)
    U = sampler_uniforms(11, 64, 64, RN)
    return idx, (U[0].to(DEV), U[1].to(DEV))


TRAINED = ("ray_transformer.", "feature_volume.cost_reg_2.", "deviation_network.variance")


@pytest.fixture(scope="module")
def stepped(initial_state, rays):
    """one model through a first step (kept: loss, gradients) and three optimizer steps in all"""
    idx, U = rays
    net = _model(initial_state)
    opt = net.configure_optimizers()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    loss, log = net.training_step(_batch(), 0, ray_idx=idx, uniforms=U)
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    opt.step()
    opt.zero_grad(set_to_none=True)
    for s in (1, 2):
        net.training_step(_batch(), s, ray_idx=idx, uniforms=U)[0].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    return net, opt, before, loss.detach().clone(), log, grads


def test_training_step_is_its_pieces_composed(initial_state, rays, stepped):
    idx, U = rays
    _, _, _, loss, log, _ = stepped
    net = _model(initial_state)
    b = _batch()
    feat, cost, depth, match = net.encode_frozen(b, cur_n_src_views=NV)
    frustums = {}
    for st in ("stage1", "stage2", "stage3"):
        f, w = net.feature_volume(b, cost[st])
        assert f.requires_grad and w.requires_grad                # the frustums are built WITH gradients
        frustums[st] = {"feature_volume": f, "weight_volume": w}
    b["depth_info"] = (depth * b["scale_factor"]).unsqueeze(0)
    r = net.infer(b, idx, feat, frustums, match_feature=match, uniforms=U)
    by_hand, parts = net.training_loss(r, b)
    assert torch.equal(by_hand.detach(), loss) and float(loss) > 0
    assert set(log) == {"train/depth_ray_coarse", "train/depth_ray_fine", "train/rgb_coarse", "train/rgb_fine", "train/loss_all",
                        "train/variance"}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and not v.requires_grad for v in log.values())
    assert torch.equal(log["train/loss_all"], loss) and torch.equal(log["train/rgb_fine"], parts["rgb_fine"])
    two = _batch()
    two["source_imgs"] = two["source_imgs"].expand(2, -1, -1, -1, -1)
    with pytest.raises(UfrError, match="B=1"):
        net.training_step(two)


def test_gradients_reach_what_trains_and_nothing_else(stepped):
    _, _, _, _, _, grads = stepped
    seen = 0
    for k, g in grads.items():
        if k.startswith(TRAINED):
            assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any()), k
            seen += 1
        else:
            assert k.startswith("transmvsnet.") or k == "pre_conv.weight", k
            assert g is None, k
    assert seen >= 60


def test_three_steps_move_what_trains_and_leave_the_frozen_encoder_bit_identical(stepped):
    net, opt, before, _, _, grads = stepped
    after = net.state_dict()
    frozen = [k for k in after if k.startswith("transmvsnet.")]
    assert any("running_mean" in k for k in frozen) and any("num_batches_tracked" in k for k in frozen)
    for k in frozen:
        assert torch.equal(after[k], before[k]), k                # parameters AND BatchNorm buffers
    for k, g in grads.items():
        assert torch.equal(after[k], before[k]) == (g is None), k
    assert all(float(opt.state[p]["step"]) == 3.0 for p in opt.state)


def test_forward_after_our_optimizer_uses_the_new_weights(initial_state, rays, stepped):
    idx, U = rays
    net, _, before, first_loss, _, _ = stepped
    new_loss = net.training_step(_batch(), 3, ray_idx=idx, uniforms=U)[0].detach()
    fresh = _model({k: v.detach().cpu() for k, v in net.state_dict().items()})
    assert torch.equal(fresh.training_step(_batch(), 3, ray_idx=idx, uniforms=U)[0].detach(), new_loss)
    assert not torch.equal(new_loss, first_loss)
    # a model whose caches are deliberately left stale: the new values written behind the version counters' back
    stale = _model(initial_state)
    assert torch.equal(stale.training_step(_batch(), 0, ray_idx=idx, uniforms=U)[0].detach(), first_loss)
    with torch.no_grad():
        for k, p in stale.named_parameters():
            p.data.copy_(net.state_dict()[k])                      # `.data`: no version bump (model.py: packed_weights)
    stale_loss = stale.training_step(_batch(), 3, ray_idx=idx, uniforms=U)[0].detach()
    assert not torch.equal(stale_loss, new_loss)
    stale.ray_transformer.invalidate_packed()
    ops._PLANES.clear()
    assert torch.equal(stale.training_step(_batch(), 3, ray_idx=idx, uniforms=U)[0].detach(), new_loss)


def test_the_ray_draw_follows_the_generator(initial_state, monkeypatch):
    net = _model(initial_state)
    drawn = []
    real = ops.select_rays
    monkeypatch.setattr(ops, "select_rays", lambda u, k: drawn.append(real(u, k)) or drawn[-1])
    losses = []
    for seed in (7, 7, 8):
        g = torch.Generator(device=DEV).manual_seed(seed)
        with torch.no_grad():
            losses.append(net.training_step(_batch(), 0, generator=g)[0])
    a, b, c = (d.cpu() for d in drawn)
    assert a.shape == (1024,) and a.unique().numel() == 1024 and int(a.min()) >= 0 and int(a.max()) < H * W
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(losses[0], losses[1]) and not torch.equal(losses[0], losses[2])


# ---------------------------------------------------------------------------------------------------------- trajectory
def _trajectory(state, rays, make_opt, steps, lr):
    idx, U = rays
    net = _model(state, lr)
    ours = net.configure_optimizers()
    opt = ours if make_opt is None else make_opt(ours.param_groups[0]["params"], lr)
    losses = []
    for s in range(steps):
        loss, _ = net.training_step(_batch(), s, ray_idx=idx, uniforms=U)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(loss.detach())
    return [float(v) for v in torch.stack(losses).double().cpu()]


@pytest.fixture(scope="module")
def scatter_spread(initial_state, rays):
    """the torch leg twice: the backward's scatter adds floats in hardware order, so two runs of the same code differ"""
    make = lambda ps, lr: torch.optim.Adam(ps, lr=lr)  # noqa: E731
    a = _trajectory(initial_state, rays, make, 5, 1e-4)
    b = _trajectory(initial_state, rays, make, 5, 1e-4)
    return a, max(abs(x - y) for x, y in zip(a, b))


def test_five_steps_with_our_adam_follow_torchs(initial_state, rays, scatter_spread):
    theirs, spread = scatter_spread
    ours = _trajectory(initial_state, rays, None, 5, 1e-4)
    diffs = [abs(x - y) for x, y in zip(ours, theirs)]
    print(f"scatter spread of the torch leg run twice {spread:.3e}; per-step |ours - torch| {['%.3e' % d for d in diffs]}; "
          f"losses {['%.6f' % v for v in ours]}")
    for d, v in zip(diffs, theirs):
        assert d <= 4.0 * spread + 1e-6 * abs(v), (d, spread, v)


def test_twenty_steps_lower_the_loss(initial_state, rays):
    """lr 1e-3, the objective fixed (same frame, rays and uniforms); weights: the seeded random encoder with
    tests/golden/ray_path_weights_seed0.npz on the ray path, as in the other tests of this file."""
    losses = _trajectory(initial_state, rays, None, 20, 1e-3)
    print("loss of step 1 %.6f, of step 20 %.6f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------------- the command
def _step_losses(logdir):
    rows = [json.loads(line) for line in open(os.path.join(logdir, "train_log.jsonl"))]
    return rows, [r["train/loss_all"] for r in rows if r["kind"] == "step"]


def test_train_command_end_to_end(tmp_path, scatter_spread):
    """Validation builds its matching features for train_n_view - 1 sources (validate.py's rule), so with the three validation
    sources of --test_ref_view 23 24 33 the run trains with --train_n_view 4: items 7 and 275 then read their first three
    source views, which the tree holds."""
    _, spread = scatter_spread
    root = G.write_tree(tmp_path)
    a = _args()
    torch.manual_seed(0)
    start = fill_state_dict(pipeline.UFOReconTraining(a, tune_convolutions=False), 21)
    start.load_state_dict(load_weights(), strict=False)
    first = {k: v.clone() for k, v in start.state_dict().items()}
    torch.save({"state_dict": first}, str(tmp_path / "start.ckpt"))
    common = ["--root_dir", root, "--split_filepath", str(tmp_path / "dtu_training" / "scans.txt"), "--load_ckpt", str(tmp_path / "start.ckpt"),
              "--batch_size", "1", "--train_items", "7", "275", "--train_n_view", "4", "--max_val_frames", "1",
              "--test_ref_view", "23", "24", "33", "--test_n_view", "3", "--view_selection_type", "best", "--depth_pos_encoding",
              "--explicit_similarity", "--mvs_depth_guide", "1", "--log_every", "1", "--seed", "3"]
    logdir = tmp_path / "log"
    assert T.main(common + ["--logdir", str(logdir), "--max_epochs", "1"]) == 0
    rows, losses = _step_losses(logdir)
    assert [r["kind"] for r in rows] == ["step", "step", "epoch"] and [r["global_step"] for r in rows] == [1, 2, 2]
    assert sorted(r["item"] for r in rows[:2]) == [7, 275] and all(np.isfinite(v) for v in losses)
    assert np.isfinite(rows[2]["val/loss_depth_fine"]) and rows[2]["frames"] == 1
    path = logdir / "checkpoints" / "epoch=00.ckpt"
    assert path.exists() and rows[2]["checkpoint"] == str(path)
    loaded = pipeline.UFOReconInference(a, tune_convolutions=False)
    load_checkpoint(loaded, str(path))                                       # strict
    trained = {k for k, _ in loaded.named_parameters() if k.startswith(TRAINED)}      # (the variance trains with the ray path)
    assert len(trained) >= 60
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, first[k]) != (k in trained), k
    ck = torch.load(str(path), map_location="cpu", weights_only=True)
    assert ck["epoch"] == 0 and ck["global_step"] == 2 and ck["monitor"]["val/loss_depth_fine"] == rows[2]["val/loss_depth_fine"]
    # --resume: the optimizer, the epoch and the step come back (no epoch left to run: nothing else happens)
    end = T.fit(common + ["--logdir", str(logdir), "--max_epochs", "1", "--resume", str(path)])
    assert end["global_step"] == 2 and end["epoch"] == 1
    saved = ck["optimizer_states"][0]["state"]
    state = end["optimizer"].state_dict()["state"]
    assert set(state) == set(saved) and len(saved) >= 60
    for i in saved:
        assert torch.equal(state[i]["exp_avg"].cpu(), saved[i]["exp_avg"]) and float(state[i]["step"]) == 2.0
    rows2, _ = _step_losses(logdir)
    assert rows2[-1]["kind"] == "resume" and rows2[-1]["global_step"] == 2
    # the same seed from scratch: the same run, up to the order of the scatter's additions
    again = tmp_path / "log2"
    assert T.main(common + ["--logdir", str(again), "--max_epochs", "1"]) == 0
    _, losses2 = _step_losses(again)
    print(f"step losses {losses} and, rerun, {losses2}; scatter spread {spread:.3e}")
    assert len(losses2) == 2
    for x, y in zip(losses, losses2):
        assert abs(x - y) <= 4.0 * spread + 1e-6 * abs(x)
