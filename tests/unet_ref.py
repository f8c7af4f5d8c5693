"""Test-side restatements for the U-Net plane kernels (csrc/conv3d_planes.hip) and the fp32 kernels beside them (csrc/conv3d.hip):

  * the launcher's geometry -- brick extents per (mode, cin), the resident workgroup count, the XCD-aware split of the bricks
    into one contiguous run per persistent workgroup (`bricks`, `run_partition`), and RUN_SHAPES: one (B, D, H, W) per
    instantiation at which a workgroup walks two or three bricks, runs cross batch elements and both remainders of the split
    are non-zero (tests/test_unet_ref.py asserts those conditions);
  * the layer itself as one torch expression (`layer`), evaluated in float64 (`layer64`: the reference) and in float32 on the
    CPU (`layer32`: the yardstick -- none of the project's kernels is one);
  * the comparison (`check`): err(kernel) < max(4 err(layer32), 1e-6) of the output scale, with a per-brick error map that names
    the brick, its workgroup and its place in the workgroup's run when it fails.

Nothing here imports the package: tests/test_unet_ref.py runs all of it without a GPU.
"""
import torch
import torch.nn.functional as F

S1, S2, T2 = 0, 1, 2                # ops.CONV3D_S1 / _S2 / _T2
MODE_NAMES = {S1: "S1", S2: "S2", T2: "T2"}
XCDS = 8

# (mode, cin) -> (TX, TY, TZ, resident workgroups): Brick<CIN, MODE> and launch_planes_t (512 = two workgroups per CU; 256 where
# the two halo planes (+ the weights' planes when they fit in 32 KiB) need more than 80 KiB of LDS)
GEOMETRY = {
    (S1, 8): (64, 4, 2, 512), (S1, 16): (32, 4, 1, 512), (S1, 32): (16, 4, 2, 512), (S1, 64): (16, 4, 1, 256),
    (S2, 8): (32, 4, 1, 512), (S2, 16): (16, 4, 1, 512), (S2, 32): (16, 4, 1, 256),
    (T2, 16): (32, 4, 1, 512), (T2, 32): (16, 4, 2, 512), (T2, 64): (16, 4, 1, 512),
}
# the layer's output channels (stride 2 doubles, transposed halves: the U-Nets' only shapes)
COUT = {(S1, 8): 8, (S1, 16): 16, (S1, 32): 32, (S1, 64): 64, (S2, 8): 16, (S2, 16): 32, (S2, 32): 64,
        (T2, 16): 8, (T2, 32): 16, (T2, 64): 32}
INSTANTIATIONS = sorted(GEOMETRY)

RUN_SHAPES = {
    (S1, 8): (7, 11, 59, 66), (S1, 16): (7, 11, 59, 17), (S1, 32): (7, 11, 59, 17), (S1, 64): (7, 9, 17, 17),
    (S2, 8): (7, 11, 65, 129), (S2, 16): (7, 11, 41, 129), (S2, 32): (7, 11, 17, 129),
    (T2, 16): (7, 11, 59, 17), (T2, 32): (7, 11, 59, 17), (T2, 64): (7, 9, 35, 17),
}


def inst_id(inst):
    return f"{MODE_NAMES[inst[0]]}-{inst[1]}"


def lds_bytes(mode, cin):
    """Dynamic LDS of an instantiation, from the kernel's own expressions (halo extents, k-steps, row tiles)."""
    TX, TY, TZ, _ = GEOMETRY[(mode, cin)]
    if mode == T2:
        halo = (TX + 1) * (TY + 1) * (TZ + 1)
    else:
        s = 2 if mode == S2 else 1
        halo = (s * (TX - 1) + 3) * (s * (TY - 1) + 3) * (s * (TZ - 1) + 3)
    ksteps = ((8 if mode == T2 else 27) * cin + 31) // 32
    ntiles = COUT[(mode, cin)] // 2 if mode == T2 else (COUT[(mode, cin)] + 15) // 16
    w_all = ksteps * ntiles * 2048
    return (w_all if w_all <= 32768 else 0) + 2 * halo * cin * 2


def out_extent(mode, dhw):
    D, H, W = dhw
    return ((D + 1) // 2, (H + 1) // 2, (W + 1) // 2) if mode == S2 else (2 * D, 2 * H, 2 * W) if mode == T2 else (D, H, W)


def grid_extent(mode, dhw):
    """The grid the bricks tile: the output grid (S1, S2), the INPUT grid for the transposed layer (eight outputs per voxel)."""
    return tuple(dhw) if mode == T2 else out_extent(mode, dhw)


def bricks(mode, cin, shape):
    """(nbx, nby, nbz, bricks per batch element, bricks of the launch) for an input of shape (B, D, H, W)."""
    B, D, H, W = shape
    TX, TY, TZ, _ = GEOMETRY[(mode, cin)]
    gz, gy, gx = grid_extent(mode, (D, H, W))
    nbx, nby, nbz = -(-gx // TX), -(-gy // TY), -(-gz // TZ)
    return nbx, nby, nbz, nbx * nby * nbz, nbx * nby * nbz * B


def grid_blocks(n_bricks, resident):
    return resident if n_bricks >= resident else -(-n_bricks // XCDS) * XCDS


def run_partition(n_bricks, resident=512):
    """[(k_begin, k_end)] per workgroup: conv3d_planes_kernel's arithmetic.  Workgroup w sits on XCD w % 8 and takes the
    (w / 8)-th share of that XCD's contiguous eighth of the bricks."""
    blocks = grid_blocks(n_bricks, resident)
    per_xcd = blocks // XCDS
    q, r = divmod(n_bricks, XCDS)
    runs = []
    for w in range(blocks):
        xcd, idx = w % XCDS, w // XCDS
        x_begin, x_count = xcd * q + min(xcd, r), q + (1 if xcd < r else 0)
        q2, r2 = divmod(x_count, per_xcd)
        k_begin = x_begin + idx * q2 + min(idx, r2)
        runs.append((k_begin, k_begin + q2 + (1 if idx < r2 else 0)))
    return runs


def brick_coords(mode, cin, shape, k):
    """brick number -> (batch element, bz, by, bx), x fastest (the kernel's brick_of)"""
    nbx, nby, nbz, _, _ = bricks(mode, cin, shape)
    bx, k = k % nbx, k // nbx
    by, k = k % nby, k // nby
    return k // nbz, k % nbz, by, bx


def brick_box(mode, cin, shape, k):
    """(batch element, slice z, slice y, slice x) of brick k in OUTPUT coordinates, cut at the output's edge."""
    TX, TY, TZ, _ = GEOMETRY[(mode, cin)]
    f = 2 if mode == T2 else 1
    Do, Ho, Wo = out_extent(mode, shape[1:])
    b, bz, by, bx = brick_coords(mode, cin, shape, k)
    return (b, slice(f * bz * TZ, min(f * (bz + 1) * TZ, Do)), slice(f * by * TY, min(f * (by + 1) * TY, Ho)),
            slice(f * bx * TX, min(f * (bx + 1) * TX, Wo)))


def where_in_runs(k, runs):
    """(workgroup, position in its run, run length) of brick k"""
    for w, (a, b) in enumerate(runs):
        if a <= k < b:
            return w, k - a, b - a
    raise ValueError(f"brick {k} is in no run")


# ---------------------------------------------------------------------------------------------------------------- the layer
def layer(x_cl, weight, mode=S1, bias=None, bn_scale=None, bn_shift=None, relu=False, skip=None, flip=False, out_ncdhw=False,
          weight2=None, dtype=torch.float64, device=None):
    """One 3x3x3 layer of the frustum U-Nets as a torch expression in ``dtype``: ``x_cl`` (B,D,H,W,cin) channel-last; ``weight``
    in the checkpoint's layout -- conv (cout,cin,3,3,3); transposed (mode T2) and ``flip`` (the data gradient of a stride-1 layer,
    on that layer's forward weight) (cin,cout,3,3,3).  y = [relu]((conv + bias) * bn_scale + bn_shift) + skip, channel-last -- or
    (B,C,D,H,W) with ``out_ncdhw``; with a second head ``weight2`` the pair (y, sigmoid(second head)), both (B,C,D,H,W)."""
    dev = x_cl.device if device is None else device
    c = lambda t: None if t is None else t.detach().to(device=dev, dtype=dtype)
    x = c(x_cl).permute(0, 4, 1, 2, 3)
    w, b = c(weight), c(bias)
    if mode == T2:
        y = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
    elif flip:
        assert mode == S1 and b is None
        y = F.conv_transpose3d(x, w, None, stride=1, padding=1)
    else:
        y = F.conv3d(x, w, b, stride=2 if mode == S2 else 1, padding=1)
    if bn_scale is not None:
        y = y * c(bn_scale).view(1, -1, 1, 1, 1) + c(bn_shift).view(1, -1, 1, 1, 1)
    if relu:
        y = torch.relu(y)
    if weight2 is not None:
        assert out_ncdhw and skip is None
        return y, torch.sigmoid(F.conv3d(x, c(weight2), None, padding=1))
    if out_ncdhw:
        return y if skip is None else y + c(skip)
    y = y.permute(0, 2, 3, 4, 1)
    return (y if skip is None else y + c(skip)).contiguous()


def layer64(x_cl, weight, mode=S1, per_element=True, **kw):
    """The reference: `layer` in float64 where the input lives; one batch element at a time (the im2col of a float64
    convolution of a whole RUN_SHAPES tensor is gigabytes)."""
    if not per_element or x_cl.shape[0] == 1:
        return layer(x_cl, weight, mode, dtype=torch.float64, **kw)
    skip = kw.pop("skip", None)
    parts = [layer(x_cl[b:b + 1], weight, mode, dtype=torch.float64, skip=None if skip is None else skip[b:b + 1], **kw)
             for b in range(x_cl.shape[0])]
    if isinstance(parts[0], tuple):
        return tuple(torch.cat(p) for p in zip(*parts))
    return torch.cat(parts)


def layer32(x_cl, weight, mode=S1, **kw):
    """The yardstick: the same expression in torch float32 on the CPU."""
    return layer(x_cl, weight, mode, dtype=torch.float32, device="cpu", **kw)


# ----------------------------------------------------------------------------------------------------------- the comparison
FLOOR = 1e-6            # of the output scale: below it a distance is fp32 rounding of the output itself, whoever computed it


def err(a, ref, keep=None):
    """Maximum absolute error over the reference's maximum (tests/test_gpu_conv3d_planes.py's metric); ``keep``: a mask of the
    elements that count, in the error and in the scale.  A NaN in ``a`` gives NaN, which is below no bound."""
    ref = ref.double()
    d = (a.to(ref.device).double() - ref).abs()
    if keep is not None:
        keep = keep.to(ref.device)
        return float(torch.where(keep, d, torch.zeros_like(d)).max() / torch.where(keep, ref.abs(), torch.zeros_like(ref)).max())
    return float(d.max() / ref.abs().max())


def bound(yardstick):
    return max(4.0 * yardstick, FLOOR)


def brick_errors(a, ref, mode, cin, shape, ncdhw=False):
    """(B, nbz, nby, nbx): per brick of the launch over the input ``shape``, the maximum absolute error over the WHOLE
    reference's maximum; a NaN counts as infinite."""
    ref = ref.double()
    d = (a.to(ref.device).double() - ref).abs()
    d = torch.nan_to_num(d, nan=float("inf"))
    d = d.amax(1) if ncdhw else d.amax(-1)                               # (B, Do, Ho, Wo)
    TX, TY, TZ, _ = GEOMETRY[(mode, cin)]
    f = 2 if mode == T2 else 1
    nbx, nby, nbz, _, _ = bricks(mode, cin, shape)
    B, Do, Ho, Wo = d.shape
    d = F.pad(d, (0, nbx * f * TX - Wo, 0, nby * f * TY - Ho, 0, nbz * f * TZ - Do))
    d = d.view(B, nbz, f * TZ, nby, f * TY, nbx, f * TX).amax((2, 4, 6))
    return d / float(ref.abs().max())


def describe_bricks(be, mode, cin, shape, limit, n=4):
    """The worst bricks of an error map, and how many bricks are over ``limit``: says whether a failure is confined to bricks
    (a run's bookkeeping) or spread over the tensor (precision)."""
    resident = GEOMETRY[(mode, cin)][3]
    total = be.numel()
    runs = run_partition(total, resident)
    flat = be.reshape(-1)                   # (b, bz, by, bx) row-major IS the kernel's brick number
    over = int((~(flat < limit)).sum())
    top = torch.argsort(flat, descending=True)[:n]
    parts = []
    for k in top.tolist():
        w, pos, length = where_in_runs(k, runs)
        b, bz, by, bx = brick_coords(mode, cin, shape, k)
        parts.append(f"brick {k} (element {b}, z {bz}, y {by}, x {bx}; workgroup {w}, place {pos} of a run of {length}) {float(flat[k]):.2e}")
    return f"{over} of {total} bricks over {limit:.2e}; worst: " + "; ".join(parts)


def check(label, got, ref64, ref32, inst=None, shape=None, ncdhw=False, keep=None):
    """THE RULE: err(got) < max(4 err(ref32), 1e-6), both against ``ref64`` and of its scale.  Prints the pair as a MEASURE
    line; with ``inst`` = (mode, cin) and the launch's input ``shape`` a failure names the bricks.  -> (err, yardstick)"""
    e, y = err(got, ref64, keep), err(ref32, ref64, keep)
    print(f"MEASURE {label}: kernel {e:.2e}  float32 torch {y:.2e}  ratio {e / max(y, 1e-30):.2f}  bound {bound(y):.2e}")
    if not e < bound(y):
        where = ""
        if inst is not None:
            g = got if keep is None else torch.where(keep.to(got.device), got, ref64.to(got.device, got.dtype))
            where = " -- " + describe_bricks(brick_errors(g, ref64, inst[0], inst[1], shape, ncdhw), inst[0], inst[1], shape, bound(y))
        raise AssertionError(f"{label}: {e:.3e} of the output scale is not below max(4 x {y:.3e}, {FLOOR:.0e}){where}")
    return e, y


def measure(label, got, ref64, ref32):
    """The same pair as a MEASURE line, nothing asserted.  -> (err, yardstick)"""
    e, y = err(got, ref64), err(ref32, ref64)
    print(f"MEASURE {label}: kernel {e:.2e}  float32 torch {y:.2e}  ratio {e / max(y, 1e-30):.2f}  (printed, not asserted)")
    return e, y


def poison(device, *shapes):
    """NaN-filled tensors of the outputs' sizes, allocated and freed, after the caching allocator has let go of every other free
    block: the blocks it hands to the next `torch.empty` of those sizes then hold NaN, not a previous call's correct values
    (with several free blocks of one size it picks the lowest address, which may be a stale one) -- a voxel the kernel under
    test does not write cannot compare equal."""
    if torch.device(device).type == "cuda":
        torch.cuda.empty_cache()
    ts = [torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=device) for shape in shapes]
    del ts


def layer_inputs(inst, shape, seed, device="cpu"):
    """Seeded inputs of one instantiation: x (a few large values: the planes' scale follows the measured maximum), the weight,
    bias, folded-BatchNorm scale / shift and a skip tensor of the output's shape."""
    mode, cin = inst
    cout = COUT[inst]
    g = torch.Generator().manual_seed(seed)
    B, D, H, W = shape
    x = torch.randn(B, D, H, W, cin, generator=g) * 2.0
    x[0, 0, 0, :3] *= 20.0
    wshape = (cin, cout, 3, 3, 3) if mode == T2 else (cout, cin, 3, 3, 3)
    w = torch.randn(wshape, generator=g) * (1.5 / (27 * cin) ** 0.5)
    bias = torch.randn(cout, generator=g)
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    skip = torch.randn(B, *out_extent(mode, (D, H, W)), cout, generator=g)
    return tuple(t.to(device) for t in (x, w, bias, sc, sh, skip))
