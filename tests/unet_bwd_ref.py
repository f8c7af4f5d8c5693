"""Test-side restatements for the backward of the trainable frustum U-Net (`feature_volume.cost_reg_2`): the weight-gradient
plane kernels (csrc/conv3d_wgrad_planes.hip) and `unet3d.CostRegNetWeightFn`.

  * the launcher's geometry -- the nine (CA, CB, S, NA, NTAP) rows and the two-heads form, brick extents in TP voxels, the job
    kinds and their decoding into channel and tap ranges, the workgroups per kind, the XCD-aware run split (`ROWS`, `kinds`,
    `kind_ranges`, `blocks_per_kind`, `run_partition`), and the two shapes every instantiation is run at: WG_SHAPE (runs of 3
    and 4 bricks crossing batch elements, bricks cut at the edge) and ONE_BRICK (seven idle workgroups per kind);
  * a layer's weight and bias gradient evaluated three ways on the CPU: `wgrad64` (float64: the reference), `wgrad32` (torch
    float32: the yardstick -- none of the project's kernels is one) and `wgrad_model` (float64 sums of the kernel's OPERAND
    arithmetic: bf16 hi + lo planes, three plane products, lo.lo dropped).  The kernel's distance from float64 is almost
    entirely that designed rounding (4e-6 .. 7e-6 of a row), so a bound on it cannot see an error inside it; its distance from
    the model is fp32 summation alone;
  * the comparison (`check_wgrad`), PER TP-CHANNEL ROW of dW[a][b][tap]: (i) |kernel - model| < max(4 |wgrad32 - wgrad64|,
    1e-6) and (ii) |kernel - wgrad64| < 2e-5, both of the row's own maximum; a failure names the worst element, its job kind
    and whether its tap shares a tile with padding taps;
  * the whole network as the reference's forward expression, for float64 / float32 autograd on the CPU.

Nothing here imports the package: tests/test_unet_bwd_ref.py runs all of it without a GPU.
"""
import copy
from types import SimpleNamespace

import torch

S1, S2, T2 = 0, 1, 2                # ops.CONV3D_S1 / _S2 / _T2
MODE_NAMES = {S1: "S1", S2: "S2", T2: "T2"}
XCDS = 8
TX, TY = 32, 4                      # a brick of TP voxels: TY TZ rows of one 32-voxel chunk; TZ = 2 (S = 1) | 1 (S = 2)

# (CA, CB, S) -> (NA, NTAP): launch_conv3d_wgrad_planes' table.  CA / CB: channels of TP / TQ; NA: 16-channel TP tiles per
# block; NTAP: taps per block
ROWS = {(8, 1, 1): (1, 27), (8, 8, 1): (1, 27), (1, 8, 1): (1, 27), (16, 16, 1): (1, 27), (32, 32, 1): (2, 9), (64, 64, 1): (2, 9),
        (16, 8, 2): (1, 27), (32, 16, 2): (2, 9), (64, 32, 2): (2, 9)}
HEADS_ROW = (8, 8, 1)               # the two heads: row CA (= 8) of the one TP tile is the 1-channel head; one kind

# the layers of CostRegNetWeight that run them, (mode, cin, cout): (TP, TQ) = (d_out, in) for the convolutions, (in, d_out) for
# the transposed one -- a stride-2 row serves a strided layer and its transposed twin in opposite roles
LAYERS = [(S1, 1, 8), (S1, 8, 8), (S1, 8, 1), (S1, 16, 16), (S1, 32, 32), (S1, 64, 64), (S2, 8, 16), (S2, 16, 32), (S2, 32, 64),
          (T2, 16, 8), (T2, 32, 16), (T2, 64, 32)]

WG_SHAPE = (3, 3, 10, 70)           # (B, Dp, Hp, Wp), the TP grid: 54 (S = 1) / 81 (S = 2) bricks on 16 / 24 workgroups per kind
ONE_BRICK = (1, 1, 3, 20)


def layer_id(layer):
    return f"{MODE_NAMES[layer[0]]}-{layer[1]}-{layer[2]}"


def row_of(layer):
    """(CA, CB, S) of a layer (mode, cin, cout)"""
    mode, cin, cout = layer
    return (cin, cout, 2) if mode == T2 else (cout, cin, 2 if mode == S2 else 1)


def in_shape(layer, tp_shape):
    """The layer INPUT's (B, D, H, W) for a TP grid: a strided layer's input is twice its d_out"""
    B, D, H, W = tp_shape
    return (B, 2 * D, 2 * H, 2 * W) if layer[0] == S2 else tuple(tp_shape)


def out_shape(layer, tp_shape):
    B, D, H, W = tp_shape
    return (B, 2 * D, 2 * H, 2 * W) if layer[0] == T2 else tuple(tp_shape)


def weight_shape(layer):
    mode, cin, cout = layer
    return (cin, cout, 3, 3, 3) if mode == T2 else (cout, cin, 3, 3, 3)


# ------------------------------------------------------------------------------------------------------------------ geometry
def cfg(row):
    """WgCfg<CA, CB, S, NA, NTAP>: what the job kinds are made of"""
    CA, CB, S = row
    NA, NTAP = ROWS[row]
    CBL = min(CB, 16)
    tpt = 16 if CB == 1 else 2 if CB == 8 else 1                # taps per 16-column tile
    return SimpleNamespace(CA=CA, CB=CB, S=S, NA=NA, NTAP=NTAP, CBL=CBL, TPT=tpt, NSLOT=-(-NTAP // tpt), TZ=2 if S == 1 else 1,
                           a_groups=-(-CA // (16 * NA)), b_blocks=CB // CBL, tap_groups=27 // NTAP)


def kinds(row):
    c = cfg(row)
    return c.a_groups * c.b_blocks * c.tap_groups


def kind_decode(row, kind):
    """blockIdx.y -> (ag, bb, tg)"""
    c = cfg(row)
    return kind // (c.tap_groups * c.b_blocks), (kind // c.tap_groups) % c.b_blocks, kind % c.tap_groups


def kind_ranges(row, kind):
    """(TP channels, TQ channels, taps) a job kind flushes, as ranges cut at the tensor's extents"""
    c = cfg(row)
    ag, bb, tg = kind_decode(row, kind)
    return (range(ag * 16 * c.NA, min((ag + 1) * 16 * c.NA, c.CA)), range(bb * c.CBL, min((bb + 1) * c.CBL, c.CB)),
            range(tg * c.NTAP, min((tg + 1) * c.NTAP, 27)))


def kind_of(row, a, b, tap):
    """the (ag, bb, tg) whose block holds dW[a][b][tap]"""
    c = cfg(row)
    return a // (16 * c.NA), b // c.CBL, tap // c.NTAP


def tap_shares_padding(row, tap):
    """True where the tap's accumulator tile also holds padding taps (27 ..): the second half of the last pair for CB = 8
    (tap 26), the second tile for CB = 1 (taps 16 .. 26)"""
    c = cfg(row)
    return c.TPT > 1 and (tap - tap % c.TPT) + c.TPT > 27


def bricks(row, tp_shape):
    """(nbx, nby, nbz, bricks per batch element, bricks of the launch)"""
    B, D, H, W = tp_shape
    tz = cfg(row).TZ
    nbx, nby, nbz = -(-W // TX), -(-H // TY), -(-D // tz)
    return nbx, nby, nbz, nbx * nby * nbz, nbx * nby * nbz * B


def blocks_per_kind(n_bricks, n_kinds):
    """launch_wgp_t: gridDim.x = min(512 / kinds, ceil(bricks / 4)) rounded up to a multiple of the 8 XCDs"""
    bx = min(512 // n_kinds, -(-n_bricks // 4))
    return -(-bx // XCDS) * XCDS


def run_partition(n_bricks, blocks):
    """[(k_begin, k_end)] per workgroup of one kind: workgroup w sits on XCD w % 8 and takes the (w / 8)-th share of that
    XCD's contiguous eighth of the bricks (the kernel's arithmetic)."""
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


def brick_box(row, tp_shape, k):
    """(batch element, slice z, slice y, slice x) of brick k in TP voxels, x fastest, cut at the grid's edge"""
    B, D, H, W = tp_shape
    tz = cfg(row).TZ
    nbx, nby, nbz, _, _ = bricks(row, tp_shape)
    bx, k = k % nbx, k // nbx
    by, k = k % nby, k // nby
    bz, b = k % nbz, k // nbz
    return b, slice(bz * tz, min((bz + 1) * tz, D)), slice(by * TY, min((by + 1) * TY, H)), slice(bx * TX, min((bx + 1) * TX, W))


# ------------------------------------------------------------------------------------------- the three evaluations of a layer
def wgrad(x_cl, d_cl, mode, dtype=torch.float64):
    """(d weight in the parameter's layout, d bias [cout]) of one plain 3x3x3 layer in ``dtype`` on the CPU: the backward that
    torch's autograd runs for the convolution (`aten::convolution_backward`; tests/test_unet_bwd_ref.py holds it against
    `.backward()` through `F.conv3d` / `F.conv_transpose3d`).  ``x_cl`` (B,D,H,W,cin), ``d_cl`` (B,Do,Ho,Wo,cout) channel-last."""
    x = x_cl.detach().to("cpu", dtype).permute(0, 4, 1, 2, 3)
    d = d_cl.detach().to("cpu", dtype).permute(0, 4, 1, 2, 3)
    cin, cout = x.shape[1], d.shape[1]
    t2 = mode == T2
    w = torch.zeros((cin, cout, 3, 3, 3) if t2 else (cout, cin, 3, 3, 3), dtype=dtype)
    s = 1 if mode == S1 else 2
    _, dw, db = torch.ops.aten.convolution_backward(d, x, w, [cout], [s] * 3, [1] * 3, [1] * 3, t2, [1 if t2 else 0] * 3, 1,
                                                    [False, True, True])
    return dw, db


def wgrad64(x_cl, d_cl, mode):
    return wgrad(x_cl, d_cl, mode, torch.float64)


def wgrad32(x_cl, d_cl, mode):
    return wgrad(x_cl, d_cl, mode, torch.float32)


def split_bf16(v):
    """split_pair_bf16: hi = bf16(v), lo = bf16(v - hi), both round to nearest even; -> (hi, lo) as float32"""
    v = v.detach().to("cpu", torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def wgrad_model(x_cl, d_cl, mode, drop=None):
    """The kernel's operand arithmetic with exact (float64) sums: dW = hi.hi + hi.lo + lo.hi of the two operands' bf16 planes;
    the bias that rides as a ones contraction = sum of hi + lo of d_out (the convolutions); the transposed layer's bias is
    channel_sum_kernel's plain fp32 sum of d_out, whose model is the exact sum.  ``drop`` = "tp_lo.tq_hi" leaves out the
    product contract3 issues first (a.p[1] b.p[0]): a mutant for the tests."""
    xh, xl = split_bf16(x_cl)
    dh, dl = split_bf16(d_cl)
    if mode == T2:                      # TP = in, TQ = d_out
        w_a, _ = wgrad64(xh, dh + dl, mode)                                          # hi.hi + hi.lo (the sum is exact in float64)
        w_b = wgrad64(xl, dh, mode)[0] if drop != "tp_lo.tq_hi" else 0.0
        bias = d_cl.detach().to("cpu", torch.float64).sum((0, 1, 2, 3))
    else:                               # TP = d_out, TQ = in
        w_a, bias = wgrad64(xh.double() + xl.double(), dh, mode)
        w_b = wgrad64(xh, dl, mode)[0] if drop != "tp_lo.tq_hi" else 0.0
        bias = bias + dl.double().sum((0, 1, 2, 3))
    return w_a + w_b, bias


def references(x_cl, d_cl, mode):
    """The three evaluations of one layer and the per-channel |max| of d_out, as one bundle for `check_wgrad`"""
    w64, b64 = wgrad64(x_cl, d_cl, mode)
    w32, b32 = wgrad32(x_cl, d_cl, mode)
    wm, bm = wgrad_model(x_cl, d_cl, mode)
    return SimpleNamespace(w64=w64, b64=b64, w32=w32, b32=b32, wm=wm, bm=bm,
                           mag=d_cl.detach().to("cpu", torch.float64).abs().amax((0, 1, 2, 3)))


def scaled(ref, s, tp_is_d_out):
    """`references` of the same layer with d_out's channel c times s[c] (or all of it times a number), every s a power of
    two: all three evaluations scale exactly, bf16 planes included, while nothing leaves the normal range (the tests keep
    far from it; test_unet_bwd_ref.py holds the identity bit for bit) -- so one CPU evaluation serves every magnitude."""
    s = torch.as_tensor(s, dtype=torch.float64).reshape(-1)
    sw = s.view(-1, 1, 1, 1, 1) if tp_is_d_out or s.numel() == 1 else s.view(1, -1, 1, 1, 1)
    f = lambda t, k: (t.double() * k).to(t.dtype)
    return SimpleNamespace(w64=f(ref.w64, sw), b64=f(ref.b64, s), w32=f(ref.w32, sw), b32=f(ref.b32, s), wm=f(ref.wm, sw),
                           bm=f(ref.bm, s), mag=ref.mag * s)


def tp_masked_to_brick(layer, tp_shape, x_cl, d_cl, k):
    """(x_cl, d_cl) with TP zero outside brick k: what one brick contributes to dW (and to the riding bias) is any evaluator
    on this pair -- the gradient is linear in TP."""
    b, z, y, x = brick_box(row_of(layer), tp_shape, k)
    tp = x_cl if layer[0] == T2 else d_cl
    m = torch.zeros_like(tp)
    m[b, z, y, x] = tp[b, z, y, x]
    return (m, d_cl) if layer[0] == T2 else (x_cl, m)


def layer_inputs(layer, tp_shape, seed, positive_input=False):
    """Seeded (x_cl, d_cl) of one layer on the CPU; ``positive_input``: |randn| + 1, so that the sums do not cancel"""
    mode, cin, cout = layer
    g = torch.Generator().manual_seed(seed)
    B, D, H, W = in_shape(layer, tp_shape)
    x = torch.randn(B, D, H, W, cin, generator=g)
    if positive_input:
        x = x.abs() + 1.0
    B, D, H, W = out_shape(layer, tp_shape)
    return x, torch.randn(B, D, H, W, cout, generator=g)


def channel_spread(c):
    """d_out channel c times 2^(-5 c), capped at 2^-40"""
    return torch.tensor([2.0 ** (-5 * min(i, 8)) for i in range(c)], dtype=torch.float64)


# ----------------------------------------------------------------------------------------------------------- the comparison
FLOOR = 1e-6            # of the row's scale: below it a distance is fp32 rounding of the sum itself, whoever computed it
ROW_BOUND = 2e-5        # the project's bound on a weight gradient against float64 (tests/test_gpu_conv3d_bwd.py), here per row


def _ratio(d, scale):
    """d / scale with 0 / 0 = 0 and x / 0 = inf (a row whose gradient is exactly zero must come out exactly zero); NaN -> inf"""
    r = torch.where(d == 0, torch.zeros_like(d), d / scale)
    return torch.nan_to_num(r, nan=float("inf"))


def row_errors(got, centre, w64):
    """[CA] and the per-element map: max over a row's (b, tap) of |got - centre|, over that row's own max |w64|"""
    w64 = w64.double()
    d = (got.detach().to("cpu", torch.float64) - centre.double()).abs()
    d = torch.nan_to_num(d, nan=float("inf"))
    e = _ratio(d.flatten(1), w64.abs().flatten(1).amax(1, keepdim=True))
    return e.amax(1), e


def tensor_error(got, w64):
    """the OLD metric (tests/test_gpu_conv3d_bwd.py:_rel): maximum error over the whole tensor's maximum"""
    return float((got.detach().to("cpu", torch.float64) - w64.double()).abs().max() / w64.double().abs().max())


def bias_errors(got, centre, b64, mag):
    """[cout]: |got - centre| of one element over the largest bias element AT THE SAME d_out MAGNITUDE: with ``mag`` the
    per-channel |max| of d_out, element c is measured against mag[c] max_c' (|b64[c']| / mag[c']) -- the whole tensor's
    maximum where the channels are alike, and no element is excused by a larger neighbour where they are not (nor held to
    its own value, which cancellation can bring near zero)."""
    b64, mag = b64.double(), mag.double()
    d = torch.nan_to_num((got.detach().to("cpu", torch.float64) - centre.double()).abs(), nan=float("inf"))
    return _ratio(d, mag * _ratio(b64.abs(), mag).max())


def bound(yardstick):
    return torch.clamp(4.0 * yardstick, min=FLOOR)


def describe(row, a, b, tap):
    ag, bb, tg = kind_of(row, a, b, tap)
    c = cfg(row)
    kind = (ag * c.b_blocks + bb) * c.tap_groups + tg
    pad = ""
    if tap_shares_padding(row, tap):
        pad = f"; tap {tap} is " + ("the last of a pair, beside padding tap 27" if c.TPT == 2 else "in the tile that ends in padding taps 27 .. 31")
    return f"dW[a={a}][b={b}][tap={tap}] in job kind {kind} (ag {ag}, bb {bb}, tg {tg}){pad}"


def _worst(emap, limit_per_row):
    """index (a, b, tap) of the element furthest over its row's limit"""
    over = emap / limit_per_row.view(-1, 1)
    i = int(torch.argmax(over))
    n = emap.shape[1]
    a, rem = divmod(i, n)
    return a, rem // 27, rem % 27


def _weight_rules(label, got_w, cw, ref, row, rules, by_column, out, fails):
    """the two rules over the slices of one axis of dW: rows (TP channels), or columns (TQ channels) with ``by_column``"""
    t = (lambda w: w.detach().to("cpu").transpose(0, 1)) if by_column else (lambda w: w)
    what = "column" if by_column else "row"
    ab = (lambda i, k: (k, i)) if by_column else (lambda i, k: (i, k))
    em, emap = row_errors(t(got_w), t(cw), t(ref.w64))
    e64, e64map = row_errors(t(got_w), t(ref.w64), t(ref.w64))
    y, _ = row_errors(t(ref.w32), t(ref.w64), t(ref.w64))
    lim = bound(y)
    ok_i = (em < lim) | (e64 < lim)
    m = dict(w_model=float(em.max()), w_64=float(e64.max()), w_32=float(y.max()), w_ratio=float((em / lim).max()))
    out.update({(k + "_col" if by_column else k): v for k, v in m.items()})
    print(f"MEASURE {label} d weight, worst {what}: kernel - model {m['w_model']:.2e}  kernel - float64 {m['w_64']:.2e}  "
          f"float32 torch - float64 {m['w_32']:.2e}  (i) at {m['w_ratio']:.2f} of its bound, (ii) at {m['w_64'] / ROW_BOUND:.2f}")
    if "i" in rules and not bool(ok_i.all()):
        i, k, tap = _worst(torch.where(ok_i.view(-1, 1), torch.zeros_like(emap), emap), lim)
        fails.append(f"(i) {int((~ok_i).sum())} of {em.numel()} {what}s over max(4 x float32, {FLOOR:.0e}); worst {describe(row, *ab(i, k), tap)}: "
                     f"{float(emap[i, k * 27 + tap]):.3e} of {what} {i}'s scale from the centre, bound {float(lim[i]):.3e}")
    if "ii" in rules and not bool((e64 < ROW_BOUND).all()):
        i, k, tap = _worst(e64map, torch.full_like(e64, ROW_BOUND))
        fails.append(f"(ii) {int((~(e64 < ROW_BOUND)).sum())} of {e64.numel()} {what}s over {ROW_BOUND:.0e}; worst {describe(row, *ab(i, k), tap)}: "
                     f"{float(e64map[i, k * 27 + tap]):.3e} of {what} {i}'s scale from float64")


def check_wgrad(label, got_w, got_b, ref, row, centre_w=None, centre_b=None, rules=("i", "ii"), bias_kernel="rides", columns=False):
    """BOTH RULES, per TP-channel row (and per bias element):
      (i)  |got - model|   < max(4 |wgrad32 - wgrad64|, 1e-6)   -- the project's rule with the model as the centre; a row (or
           the bias) that meets the rule with float64 ITSELF as the centre, as the project states it everywhere else, meets
           it too: a kernel more exact than its model is not wrong;
      (ii) |got - wgrad64| < 2e-5                                -- the project's bound on a weight gradient.
    ``ref`` = `references(...)`; ``row`` = (CA, CB, S); ``got_b`` None: no bias.  ``centre_*`` replace the model in (i) (what
    another launch of the same kernel gave: equal but for the order of the atomics).  ``columns``: the same two rules once
    more per TQ-channel COLUMN, each against its own maximum -- for the transposed layer, whose d_out is TQ: there a small
    d_out channel is a column, and every row's maximum sits in the largest one.  Prints MEASURE lines; a failure names the
    worst element, its job kind and its tap's tile.  -> dict of the worst measured values"""
    cw = ref.wm if centre_w is None else centre_w
    out, fails = {}, []
    _weight_rules(label, got_w, cw, ref, row, rules, False, out, fails)
    if columns:
        _weight_rules(label, got_w, cw, ref, row, rules, True, out, fails)
    if got_b is not None:
        cb = ref.bm if centre_b is None else centre_b
        bm_, b64_, by = bias_errors(got_b, cb, ref.b64, ref.mag), bias_errors(got_b, ref.b64, ref.b64, ref.mag), bias_errors(ref.b32, ref.b64, ref.b64, ref.mag)
        blim = float(bound(by.max()))
        out.update(b_model=float(bm_.max()), b_64=float(b64_.max()), b_32=float(by.max()), b_ratio=float(bm_.max()) / blim)
        print(f"MEASURE {label} d bias ({bias_kernel}), worst element: kernel - model {out['b_model']:.2e}  kernel - float64 {out['b_64']:.2e}  "
              f"float32 torch - float64 {out['b_32']:.2e}  (i) at {out['b_ratio']:.2f} of its bound, (ii) at {out['b_64'] / ROW_BOUND:.2f}")
        if "i" in rules and not (float(bm_.max()) < blim or float(b64_.max()) < blim):
            c = int(torch.argmax(bm_))
            fails.append(f"(i) d bias[{c}] (job kind of ag {c // (16 * cfg(row).NA) if bias_kernel == 'rides' else '-'}, bb 0, tg 0): "
                         f"{float(bm_[c]):.3e} of its scale from the centre, bound {blim:.3e}")
        if "ii" in rules and not float(b64_.max()) < ROW_BOUND:
            c = int(torch.argmax(b64_))
            fails.append(f"(ii) d bias[{c}]: {float(b64_[c]):.3e} of its scale from float64, bound {ROW_BOUND:.0e}")
    if fails:
        raise AssertionError(f"{label}: " + " | ".join(fails))
    return out


# ---------------------------------------------------------------------------------------------------------- the whole network
def cost_reg_net_weight(m, x):
    """CostRegNetWeight.forward as the reference writes it (oracle/cascade_oracle.py:cost_reg_net_weight; no activation between
    the convolutions) on the module's own layers, whatever their dtype -> (features, sigmoid(weights))"""
    c0 = m.conv0(x)
    c2 = m.conv2(m.conv1(c0))
    c4 = m.conv4(m.conv3(c2))
    y = m.conv6(m.conv5(c4))
    y = c4 + m.conv7(y)
    y = c2 + m.conv9(y)
    y = c0 + m.conv11(y)
    return m.features(y), torch.sigmoid(m.weights(y))


def net_gradients(m, x, loss_of, dtype, frozen=(), x_grad=True):
    """{parameter name: gradient, "x": d x} of ``loss_of(features, weights)`` by autograd through the expression above, in
    ``dtype`` on the CPU, on a DEEP COPY of the module (the caller's parameters and their .grad stay untouched).  ``loss_of``
    gets tensors of ``dtype`` on the CPU and casts its own constants with `.to(feat)`."""
    mc = copy.deepcopy(m).to("cpu", dtype)
    for k, p in mc.named_parameters():
        p.grad = None
        p.requires_grad_(k not in frozen)
    xc = x.detach().to("cpu", dtype).clone().requires_grad_(x_grad)
    loss_of(*cost_reg_net_weight(mc, xc)).backward()
    # (a parameter the loss does not reach has the gradient zero, not none: what the kernels' backward returns for it)
    out = {k: (None if not p.requires_grad else torch.zeros_like(p) if p.grad is None else p.grad.clone()) for k, p in mc.named_parameters()}
    out["x"] = None if xc.grad is None else xc.grad.clone()
    return out


def tensor_rel(a, ref):
    """maximum error over the reference's maximum (0 / 0 = 0), NaN -> inf: the project's per-tensor metric"""
    d = torch.nan_to_num((a.detach().to("cpu", torch.float64) - ref.double()).abs(), nan=float("inf")).max()
    s = ref.double().abs().max()
    return 0.0 if float(d) == 0.0 else float(d / s)


def rows_close(label, got, centre, ref64, ref32):
    """Rule (i) between two results of the SAME kernels (a frozen neighbour, a second launch): per row of a weight (dim 0),
    per whole tensor otherwise, |got - centre| < max(4 |ref32 - ref64|, 1e-6) of the row's scale in ``ref64``."""
    two_d = lambda t: t.detach().to("cpu", torch.float64).reshape(t.shape[0] if t.dim() > 1 else 1, -1)
    g, c, r64, r32 = two_d(got), two_d(centre), two_d(ref64), two_d(ref32)
    scale = r64.abs().amax(1, keepdim=True)
    e = _ratio(torch.nan_to_num((g - c).abs(), nan=float("inf")), scale).amax(1)
    lim = bound(_ratio((r32 - r64).abs(), scale).amax(1))
    if not bool((e < lim).all()):
        a = int(torch.argmax(e / lim))
        raise AssertionError(f"{label}: row {a} differs by {float(e[a]):.3e} of its scale, bound {float(lim[a]):.3e}")
    return float(e.max())
