"""Ray sharding + tile all-gather, covered on CPU with 2 gloo processes (the N>1 path of bench.py)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from uforecon_amd.dist import RayShard, all_gather_tiles, allreduce_gradients


@pytest.mark.parametrize("H,W,world", [(512, 640, 8), (63, 10, 4), (5, 3, 2), (7, 3, 8)])
def test_row_tiles_partition_the_frame(H, W, world):
    seen = torch.zeros(H * W, dtype=torch.int32)
    for r in range(world):
        s = RayShard(H, W, world, r)
        idx = s.ray_indices("cpu")
        assert idx.numel() == s.n_rays <= s.max_rays
        if idx.numel():
            assert int(idx[0]) % W == 0 and bool((idx[1:] - idx[:-1] == 1).all())  # whole rows, contiguous
        seen[idx] += 1
    assert bool((seen == 1).all())


def _worker(rank, world, port, H, W, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = RayShard(H, W, world, rank)
        idx = shard.ray_indices("cpu")
        depth = idx.float() * 0.5            # a function of the global ray index
        rgb = torch.stack([idx.float(), idx.float() + 1, idx.float() + 2], 1)
        d, c = all_gather_tiles(depth, rgb, shard)
        full = torch.arange(H * W).float()
        ok = torch.equal(d.reshape(-1), full * 0.5) and torch.equal(c.reshape(-1, 3)[:, 2], full + 2)
        q.put((rank, bool(ok), tuple(d.shape), tuple(c.shape)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("H,W", [(8, 6), (7, 5)])
def test_all_gather_tiles_world2_gloo(H, W):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, H, W, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, ds, cs in res:
        assert ok and ds == (H, W) and cs == (H, W, 3)


def _grad_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(0)
        # the per-ray parameter shapes (scalar variance included); then a parameter whose gradient is None on rank 1 only
        # (unused there this step: the bucket must still have the same length on every rank), one that is None everywhere,
        # and a frozen one (not in the bucket)
        shapes = [(32, 8), (32,), (160, 160), (80, 160), (88,), (1, 80), ()]
        params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        lopsided, unused = torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3))
        frozen = torch.nn.Parameter(torch.zeros(4), requires_grad=False)
        for i, p in enumerate(params):
            p.grad = torch.full(p.shape, float(rank + 1)) * (i + 1) + torch.arange(p.numel()).float().view(p.shape)
        if rank == 0:
            lopsided.grad = torch.full((5,), 6.0)
        n = allreduce_gradients(params + [lopsided, unused, frozen])
        ok = n == sum(p.numel() for p in params) + 5 + 3 and frozen.grad is None
        for i, p in enumerate(params):
            want = torch.full(p.shape, (1 + world) / 2.0) * (i + 1) + torch.arange(p.numel()).float().view(p.shape)
            ok = ok and torch.allclose(p.grad, want)
        ok = ok and torch.allclose(lopsided.grad, torch.full((5,), 6.0 / world)) and bool((unused.grad == 0).all())
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_gradient_allreduce_world2_gloo():
    """Data-parallel training step (BASELINE configs[4]): one flat all-reduce averages every gradient over the ranks."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_grad_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res)


def _bcast_worker(rank, world, port, q):
    """Frame k's tile all-gather (default group) while frame k+1's frustum broadcast is still in flight on ITS OWN group
    (uforecon_amd/evalset.py: EvalLoop.bcast_group): on one group the all-gather would queue behind the broadcast."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = dist.new_group()
        big = torch.full((48 << 20,), float(rank))                 # 192 MB: frame k+1's frustums, owner = rank 1
        work = dist.broadcast(big, src=1, group=g, async_op=True)
        shard = RayShard(8, 6, world, rank)
        idx = shard.ray_indices("cpu")
        d, _ = all_gather_tiles(idx.float(), None, shard)          # frame k's depth map
        pending_when_gathered = not work.is_completed()
        work.wait()
        ok = torch.equal(d.reshape(-1), torch.arange(48).float()) and bool((big == 1.0).all())
        q.put((rank, bool(ok), bool(pending_when_gathered)))
    finally:
        dist.destroy_process_group()


def test_all_gather_is_not_queued_behind_the_frustum_broadcast_world2_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res)
    # the depth map was complete while the 192 MB broadcast was still moving, on at least one of the two ranks (a loaded
    # host can finish the broadcast first on one of them; both would mean the two collectives were serialised)
    assert any(pending for _, _, pending in res)


def _two_rank_backend():
    """(backend, env) of the 2-rank launcher tests: RCCL with one device per rank where the box has two, else both ranks on
    the one device over gloo (UFR_BENCH_SHARE_GPU: diagnostics mode of the bench scripts)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if torch.cuda.device_count() >= 2:
        return "nccl", env
    env["UFR_BENCH_SHARE_GPU"] = "1"
    return "gloo", env


@pytest.mark.gpu
def test_two_rank_bench_renders_the_one_rank_frame(tmp_path):
    """The real N > 1 path of bench.py (launcher -> one process per rank -> row-tile sharding -> all-gather) with 2 ranks
    sharing this box's single GPU over gloo: the gathered (H,W) depth map must equal the 1-rank frame bit for bit, and
    rank 0 must report every rank's kernel split and all-gather time."""
    import json
    import subprocess
    import sys

    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--height", "64", "--width", "96", "--steps", "1", "--warmup", "1", "--fixed-uniforms", "7", "--full",
              "--no-cpu-baseline", "--no-gpu-eager-baseline", "--chunk", "2048"]
    backend, env = _two_rank_backend()
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--details", str(tmp_path / "one.json"), "--dump-depth", str(tmp_path / "d1.npy"),
                          *common], capture_output=True, text=True, env=env, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--backend", backend,
                          "--details", str(tmp_path / "two.json"), "--dump-depth", str(tmp_path / "d2.npy"), *common], capture_output=True, text=True, env=env, timeout=900)
    assert two.returncode == 0, two.stderr[-2000:]
    d1, d2 = np.load(tmp_path / "d1.npy"), np.load(tmp_path / "d2.npy")
    assert d1.shape == d2.shape == (64, 96)
    assert np.array_equal(d1, d2)
    out = [ln for ln in two.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == 1 and len(out[0]) < 4096              # ONE short headline on stdout; the tables are in --details
    line = json.loads(out[0])
    assert line["n_gpus"] == 2 and [r[:2] for r in line["config"]["per_rank"]] == [[0, 32 * 96], [1, 32 * 96]]
    full = json.load(open(tmp_path / "two.json"))
    assert full["value"] == pytest.approx(line["value"], rel=1e-8) and len(full["config"]["per_rank"]) == 2
    for r in full["config"]["per_rank"]:
        assert r["rays"] == 32 * 96 and "view_transformer" in r["kernel_ms_per_frame"] and r["all_gather_ms_per_step"] >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("producers", ["replicated", "sharded"])
def test_two_rank_evaluation_loop_renders_the_one_rank_depth_maps(tmp_path, producers):
    """BASELINE configs[2] through the real launcher path: the evaluation loop over several frames -- per-frame producers one
    frame ahead on a side stream, this rank's row tile through ufr_render_rays, all-gather -- with 2 ranks sharing this box's
    single GPU over gloo, the producers either replicated on both ranks or dealt over the ranks and broadcast: every depth
    map must equal the 1-rank loop's bit for bit (rays are independent, the producers deterministic)."""
    import json
    import subprocess
    import sys

    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--config", "c3", "--frames", "4", "--height", "128", "--width", "160", "--fixed-uniforms", "5", "--chunk", "2048",
              "--producers", producers]
    backend, env = _two_rank_backend()
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--details", str(tmp_path / "one.json"), "--dump-depths", str(tmp_path / "d1.npy"),
                          *common], capture_output=True, text=True, env=env, timeout=900)
    assert one.returncode == 0, one.stderr[-2000:]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--backend", backend,
                          "--details", str(tmp_path / "two.json"), "--dump-depths", str(tmp_path / "d2.npy"), *common], capture_output=True, text=True, env=env, timeout=1200)
    assert two.returncode == 0, two.stderr[-2000:]
    d1, d2 = np.load(tmp_path / "d1.npy"), np.load(tmp_path / "d2.npy")
    assert d1.shape == d2.shape == (4, 128, 160)
    assert np.isfinite(d1).all() and len({d1[k].tobytes() for k in range(4)}) == 4       # four different frames
    assert np.array_equal(d1, d2)
    out = [ln for ln in two.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == 1 and len(out[0]) < 4096
    head = json.loads(out[0])
    assert head["n_gpus"] == 2 and head["config"]["frames"] == 4 and len(head["config"]["per_rank"]) == 2
    line = json.load(open(tmp_path / "two.json"))
    assert line["n_gpus"] == 2 and line["config"]["frames"] == 4 and len(line["config"]["per_rank"]) == 2
    encodes = sorted(r["encodes"] for r in line["config"]["per_rank"])
    assert encodes == ([4, 4] if producers == "replicated" else [2, 2])
    for k in ("encode_frame_ms", "ray_path_ms_per_frame_rank0", "depth_map_ms_per_frame_inclusive", "ray_path_only_rays_per_s"):
        assert line["config"][k] > 0


@pytest.mark.gpu
def test_two_rank_training_step_allreduces_to_the_mean(tmp_path):
    """The data-parallel leg of BASELINE configs[4] through the real launcher path (torch.distributed.run -> one process per
    rank -> tools/bench_train.py --gpus 2), both ranks on this box's single GPU over gloo: every rank trains on its own
    frame / rays, and the parameter gradients after the flat all-reduce must equal the MEAN of the two ranks' own
    gradients (each reproduced by a single-process run on that rank's data).  Rank 0 reports per-rank step and
    all-reduce times."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tools", "bench_train.py")
    common = ["--height", "64", "--width", "96", "--rays", "128", "--steps", "1", "--warmup", "0", "--fixed-seed", "3",
              "--no-cpu-baseline"]
    backend, env = _two_rank_backend()
    for r in (0, 1):
        one = subprocess.run([sys.executable, script, "--gpus", "1", "--data-rank", str(r), "--dump-grads", str(tmp_path / f"g{r}.pt"),
                              *common], capture_output=True, text=True, env=env, timeout=600)
        assert one.returncode == 0, one.stderr[-2000:]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), script, "--gpus", "2", "--backend", backend, "--dump-grads",
                          str(tmp_path / "g2.pt"), *common], capture_output=True, text=True, env=env, timeout=900)
    assert two.returncode == 0, two.stderr[-2000:]
    g0, g1, g2 = (torch.load(tmp_path / f"g{k}.pt") for k in ("0", "1", "2"))
    assert set(g0) == set(g1) == set(g2) and len(g2) >= 40
    differ = 0
    for k in g2:
        mean = 0.5 * (g0[k] + g1[k])
        scale = float(mean.abs().max()) + 1e-12
        # float atomics reorder sums between runs (a tensor whose entries are small differences of large sums -- the first
        # pre_sim_mlp layer -- moved by 6e-5 of its scale in most runs, past 1e-4 in one of ~10; the gradient tolerance
        # itself is 1e-3)
        assert float((g2[k] - mean).abs().max()) <= 3e-4 * scale + 1e-9, k
        differ += int(float((g0[k] - g1[k]).abs().max()) > 1e-3 * scale)
    assert differ > 30          # the ranks really trained on different data
    line = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and len(line["config"]["per_rank"]) == 2
    for r in line["config"]["per_rank"]:
        assert r["all_reduce_ms_per_step"] >= 0 and "view_dgrad" in r["kernel_ms_per_step"] and r["wall_ms_per_step"] > 0


@pytest.mark.gpu
def test_bench_line_contract(tmp_path):
    """One JSON line with the fields the driver and the review read (metric / value / unit / n_gpus / steps / warmup /
    ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload, roofline, cpu_baseline,
    gpu_eager_baseline), on a small frame so that it runs in seconds."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--height", "64", "--width", "96", "--steps", "2", "--warmup", "1",
                        "--full", "--eager-chunks", "1"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "gpu_eager_baseline"):
        assert k in d, k
    assert d["unit"] == "rays/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["data"] == "synthetic" and d["dtype"] == "f32" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 64 * 96 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-6 * rf["frac"]
    assert abs(rf["peak"] - 2516.6 / 3) < 1e-4 and rf["kernel"] == "view_transformer_kernel" and rf["avg_launch_ms"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "rays/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert d["gpu_eager_baseline"]["value"] > 0 and abs(d["vs_baseline"] - d["value"] / d["gpu_eager_baseline"]["value"]) < 1e-6 * d["vs_baseline"]
