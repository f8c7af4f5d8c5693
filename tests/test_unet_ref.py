"""tests/unet_ref.py pinned, without a GPU: the restated geometry of csrc/conv3d_planes.hip (every brick in exactly one run, the
conditions RUN_SHAPES must meet), the float64 / float32 layer expressions against each other and against autograd, and the
comparison of tests/test_gpu_conv3d_runs.py run on float64 rounded to float32 (it passes) and on deliberately wrong results of
the kind a persistent workgroup can produce in the second half of its run (each must fail, and the message must name the brick)."""
import functools

import pytest
import torch

import unet_ref as R
from unet_ref import S1, S2, T2


def test_resident_workgroups_follow_the_lds_footprint():
    """launch_planes_t: 256 workgroups where the dynamic LDS is above 80 KiB (one per CU), else 512; nothing above the CU's 160."""
    for (mode, cin), (_, _, _, resident) in R.GEOMETRY.items():
        lds = R.lds_bytes(mode, cin)
        assert lds <= 160 * 1024
        assert resident == (256 if lds > 80 * 1024 else 512), (mode, cin, lds)


@pytest.mark.parametrize("resident", [512, 256])
def test_run_partition_covers_every_brick_exactly_once(resident):
    for n in range(1, 4001):
        runs = R.run_partition(n, resident)
        assert len(runs) % R.XCDS == 0 and len(runs) == (resident if n >= resident else -(-n // 8) * 8)
        assert all(b >= a for a, b in runs)
        chain = sorted(r for r in runs if r[1] > r[0])
        assert chain[0][0] == 0 and chain[-1][1] == n, n
        assert all(chain[i][1] == chain[i + 1][0] for i in range(len(chain) - 1)), n      # no gap, no brick twice
        if n < resident:                     # the state the suite pinned before: at most one brick per workgroup
            assert max(b - a for a, b in runs) == 1
        # a workgroup's XCD (w % 8) owns one contiguous eighth
        for xcd in range(R.XCDS):
            mine = [r for r in runs[xcd::R.XCDS] if r[1] > r[0]]
            assert all(mine[i][1] == mine[i + 1][0] for i in range(len(mine) - 1)), (n, xcd)


def test_brick_numbering_is_row_major_over_element_z_y_x():
    inst, shape = (S2, 16), R.RUN_SHAPES[(S2, 16)]
    nbx, nby, nbz, per, total = R.bricks(*inst, shape)
    seen = [R.brick_coords(*inst, shape, k) for k in range(total)]
    assert seen == [(b, z, y, x) for b in range(shape[0]) for z in range(nbz) for y in range(nby) for x in range(nbx)]
    assert per * shape[0] == total


@pytest.mark.parametrize("inst", R.INSTANTIATIONS, ids=R.inst_id)
def test_run_shapes_walk_runs_across_elements_with_both_remainders(inst):
    mode, cin = inst
    shape = R.RUN_SHAPES[inst]
    B, D, H, W = shape
    TX, TY, TZ, resident = R.GEOMETRY[inst]
    nbx, nby, nbz, per, total = R.bricks(mode, cin, shape)
    assert per < resident                                        # one element alone: one brick per workgroup
    assert all(b - a <= 1 for a, b in R.run_partition(per, resident))
    assert total > 2.2 * resident
    assert total % 8 != 0                                        # the XCD split has a remainder ...
    runs = R.run_partition(total, resident)
    lengths = {b - a for a, b in runs}
    assert len(lengths) > 1 and max(lengths) >= 3                # ... and so has the split inside an XCD
    assert any((total // 8 + (1 if xcd < total % 8 else 0)) % (resident // 8) for xcd in range(8))
    gz, gy, gx = R.grid_extent(mode, (D, H, W))
    assert gx % TX and gy % TY                                   # bricks cut off at the volume's edge
    if mode == S2:
        assert D % 2 and H % 2 and W % 2
    # a run crosses from one batch element into the next
    assert any(a // per != (b - 1) // per for a, b in runs if b > a)
    # one batch element is a raw buffer descriptor: 31-bit byte offsets
    assert D * H * W * cin * 4 < 2 ** 31
    print(f"{R.inst_id(inst)} {shape}: {total} bricks, run lengths {sorted(lengths)}")


# ------------------------------------------------------------------------------------------------------------ the references
def test_layer_expressions_agree_and_the_flip_form_is_the_data_gradient():
    torch.manual_seed(0)
    for inst in [(S1, 8), (S2, 16), (T2, 16)]:
        x, w, bias, sc, sh, skip = R.layer_inputs(inst, (2, 3, 7, 9), seed=1)
        kw = dict(bias=bias, skip=skip) if inst[0] == T2 else dict(bias=bias, bn_scale=sc, bn_shift=sh, relu=True, skip=skip)
        r64, r32 = R.layer64(x, w, inst[0], **kw), R.layer32(x, w, inst[0], **kw)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert r64.shape == (2, *R.out_extent(inst[0], (3, 7, 9)), R.COUT[inst])
        assert torch.equal(r64, R.layer64(x, w, inst[0], per_element=False, **kw))
        assert 0 < R.err(r32, r64) < 2e-6
    # flip: the data gradient of a stride-1 layer on its forward weight
    xg = torch.randn(1, 8, 3, 5, 6, dtype=torch.float64, requires_grad=True)
    w = torch.randn(8, 8, 3, 3, 3, dtype=torch.float64)
    dy = torch.randn(1, 8, 3, 5, 6, dtype=torch.float64)
    (torch.nn.functional.conv3d(xg, w, padding=1) * dy).sum().backward()
    got = R.layer64(dy.permute(0, 2, 3, 4, 1).contiguous(), w, S1, flip=True)
    assert R.err(got, xg.grad.permute(0, 2, 3, 4, 1)) < 1e-14
    # the two heads, (B,C,D,H,W) and sigmoid on the second
    x = torch.randn(2, 3, 5, 6, 8)
    wf, ww = torch.randn(8, 8, 3, 3, 3), torch.randn(1, 8, 3, 3, 3)
    f, s = R.layer64(x, wf, S1, out_ncdhw=True, weight2=ww)
    assert f.shape == (2, 8, 3, 5, 6) and s.shape == (2, 1, 3, 5, 6) and 0 < float(s.min()) and float(s.max()) < 1
    assert torch.equal(f, R.layer64(x, wf, S1, out_ncdhw=True)) and torch.equal(s, torch.sigmoid(R.layer64(x, ww, S1, out_ncdhw=True)))
    assert torch.equal(f.permute(0, 2, 3, 4, 1), R.layer64(x, wf, S1))


def test_brick_error_map_finds_the_brick():
    inst, shape = (T2, 16), (2, 3, 9, 40)
    ref = torch.randn(2, 6, 18, 80, 8, dtype=torch.float64)
    nbx, nby, nbz, per, total = R.bricks(*inst, shape)
    for k in (0, 7, total - 1):
        bad = ref.clone()
        b, sz, sy, sx = R.brick_box(*inst, shape, k)
        bad[b, sz, sy, sx] += 1.0
        be = R.brick_errors(bad, ref, *inst, shape)
        assert be.shape == (2, nbz, nby, nbx) and int(be.reshape(-1).argmax()) == k and int((be > 0).sum()) == 1
    nan = ref.clone()
    nan[1, 5, 17, 79, 3] = float("nan")
    be = R.brick_errors(nan, ref, *inst, shape)
    assert int(be.reshape(-1).argmax()) == total - 1 and float(be.max()) == float("inf")
    assert not R.err(nan, ref) < 1.0                         # a NaN is below no bound


REJECT = [(S1, 8), (S2, 16), (T2, 16)]


@functools.lru_cache(maxsize=None)
def _reject_case(inst):
    shape = R.RUN_SHAPES[inst]
    x, w, bias, sc, sh, skip = R.layer_inputs(inst, shape, seed=5)
    kw = dict(bias=bias, skip=skip)
    return shape, x, w, kw, R.layer64(x, w, inst[0], **kw), R.layer32(x, w, inst[0], **kw)


def _late_brick(inst, shape):
    """A brick in the second half of a run of three whose previous brick is in the same batch element."""
    _, _, _, per, total = R.bricks(*inst, shape)
    for a, b in R.run_partition(total, R.GEOMETRY[inst][3]):
        if b - a >= 3 and (b - 1) // per == (b - 2) // per:
            return b - 1
    raise AssertionError("no such run")


@pytest.mark.parametrize("inst", REJECT, ids=R.inst_id)
def test_comparison_accepts_float64_rounded_to_float32(inst):
    shape, x, w, kw, r64, r32 = _reject_case(inst)
    e, y = R.check(f"{R.inst_id(inst)} rounded float64", r64.float(), r64, r32, inst, shape)
    assert e <= 2.0 ** -24 and y > 0


@pytest.mark.parametrize("wrong", ["left zero", "left NaN", "the neighbour brick's values", "the previous brick's halo"])
@pytest.mark.parametrize("inst", REJECT, ids=R.inst_id)
def test_comparison_rejects_a_wrong_brick_late_in_a_run_and_names_it(inst, wrong):
    mode, cin = inst
    shape, x, w, kw, r64, r32 = _reject_case(inst)
    k = _late_brick(inst, shape)
    b, sz, sy, sx = R.brick_box(mode, cin, shape, k)
    bad = r64.float()
    if wrong == "left zero":                               # the brick never written, into fresh memory
        bad[b, sz, sy, sx] = 0.0
    elif wrong == "left NaN":                              # ... into a poisoned block
        bad[b, sz, sy, sx] = float("nan")
    elif wrong == "the neighbour brick's values":          # brick k - 1 computed again and stored at brick k's place
        pb, pz, py, px = R.brick_box(mode, cin, shape, k - 1)
        src = bad[pb, pz, py, px]
        dst = bad[b, sz, sy, sx]
        n = [min(p, q) for p, q in zip(src.shape, dst.shape)]
        dst[:n[0], :n[1], :n[2]] = src[:n[0], :n[1], :n[2]].clone()
    else:                                                  # brick k's sums over the halo staged for brick k - 1; own bias and skip
        TX, TY, TZ, _ = R.GEOMETRY[inst]
        s = 2 if mode == S2 else 1
        (_, z1, y1, x1), (_, z0, y0, x0) = R.brick_coords(mode, cin, shape, k), R.brick_coords(mode, cin, shape, k - 1)
        xs = torch.roll(x[b:b + 1], shifts=(s * TZ * (z1 - z0), s * TY * (y1 - y0), s * TX * (x1 - x0)), dims=(1, 2, 3))
        stale = R.layer64(xs, w, mode, bias=kw["bias"], skip=kw["skip"][b:b + 1])
        bad[b, sz, sy, sx] = stale[0, sz, sy, sx].float()
    w_, pos, length = R.where_in_runs(k, R.run_partition(R.bricks(mode, cin, shape)[4], R.GEOMETRY[inst][3]))
    assert pos >= 2 and length >= 3
    with pytest.raises(AssertionError, match=rf"1 of \d+ bricks over .*worst: brick {k} \(element {b}, .*workgroup {w_}, place {pos} of a run of {length}\)"):
        R.check(f"{R.inst_id(inst)} {wrong}", bad, r64, r32, inst, shape)


def test_outlier_mask_keeps_the_rule_outside_the_neighbourhood():
    """`keep`: error and scale over the kept voxels only -- a wrong value inside the mask's hole does not count, one outside does."""
    ref = torch.randn(1, 4, 6, 8, 8, dtype=torch.float64)
    keep = torch.ones(ref.shape, dtype=torch.bool)
    keep[0, 1:4, 2:5, 3:6] = False
    ref[0, 2, 3, 4] = 1e4
    got = ref.float()
    got[0, 2, 3, 4, 0] += 100.0
    r32 = (ref * (1 + 1e-7)).float()
    R.check("hole", got, ref, r32, keep=keep)
    assert R.err(got, ref) > 1e-3 and R.err(got, ref, keep) < 1e-7
    got[0, 0, 0, 0, 0] += 1e-3
    with pytest.raises(AssertionError):
        R.check("outside", got, ref, r32, keep=keep)
