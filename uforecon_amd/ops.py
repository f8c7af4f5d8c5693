"""Torch-facing wrappers over the C ABI (include/ufr.h).

torch is plumbing here: it owns device memory (caching allocator) and the current HIP stream;
every computation is a libufr.so kernel.  All wrappers validate device / dtype / contiguity the
way TORCH_CHECK would and raise ``UfrError`` with the library's message on failure.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import UfrError

# state_dict key (reference names) for every pointer of ufr_raw_weights, in declaration order
_RT = "ray_transformer."
_VT = _RT + "density_view_transformer.layers.0."
_RY = _RT + "density_ray_transformer.layers.0."
RAW_WEIGHT_KEYS = (
    [_RT + f"pre_sim_mlp.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    + [_VT + k for k in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight",
                         "mlp.2.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
    + [_RY + k for k in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight",
                         "mlp.2.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
    + [_RT + f"DensityMLP.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    + [_RT + f"linear_radianceweight_1_softmax.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    + [_RT + "viewToken.view_token", "deviation_network.variance"]
)
RAW_WEIGHT_SHAPES = (
    [(32, 8), (32,), (32, 32), (32,), (16, 32), (16,)]
    + [(80, 80)] * 4 + [(160, 160), (80, 160)] + [(80,)] * 4
    + [(88, 88)] * 4 + [(176, 176), (88, 176)] + [(88,)] * 4
    + [(32, 88), (32,), (16, 32), (16,), (1, 16), (1,)]
    + [(16, 83), (16,), (8, 16), (8,), (1, 8), (1,)]
    + [(1, 80), ()]
)
assert len(RAW_WEIGHT_KEYS) == 40 == len(RAW_WEIGHT_SHAPES)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> int:
    if not isinstance(t, torch.Tensor):
        raise UfrError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise UfrError(f"{name}: must live on the GPU (got {t.device}); the per-ray path has no CPU implementation")
    _typed(t, name, dtype)
    return t.data_ptr()


def _typed(t: torch.Tensor, name: str, dtype) -> None:
    """the checks of ``_dev`` that do not ask where the tensor lives"""
    if t.dtype != dtype:
        raise UfrError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise UfrError(f"{name}: must be contiguous")


def _opt(t: Optional[torch.Tensor], name: str) -> Optional[int]:
    return None if t is None else _dev(t, name)


PRECISION_DEFAULT, PRECISION_FP32, PRECISION_16BIT = -1, 0, 1


def resolve_precision(precision: Optional[int]) -> int:
    """An explicit matrix precision (include/ufr.h: UFR_PRECISION_FP32 / _16BIT) for a call: None / PRECISION_DEFAULT
    resolve to the process default NOW, so that the value recorded with a forward is what its backward gets."""
    if precision is None or precision == PRECISION_DEFAULT:
        return get_matrix_precision()
    if precision not in (PRECISION_FP32, PRECISION_16BIT):
        raise UfrError(f"unknown matrix precision {precision!r}")
    return int(precision)


def status_poll(synchronize: bool = True, mask: int = 7) -> int:
    """ufr_status_poll_bits: raises UfrError when one of the ``mask`` bits of the device's sticky range status is set (1: an
    activation beyond the fp16x3 planes, 2: NaN among a transformer kernel's inputs, 4: a weight outside the planes'
    range), clearing those bits.  With ``synchronize=False`` only what an earlier launch has already delivered is reported
    (no host synchronisation)."""
    flags = C.c_int32(0)
    _lib.check(_lib.load().ufr_status_poll_bits(_stream(), int(bool(synchronize)), int(mask), C.byref(flags)), "ufr_status_poll")
    return int(flags.value)


import itertools

_PACK_SERIAL = itertools.count(1)


class PackedWeights:
    """ufr_raw_weights (pointers into the live parameters) + the MFMA-ordered packed copy.  ``precision``: the matrix
    precision the calls made with these weights use (None = the process default at call time).  ``input_abs_max``: an
    OPTIONAL floor of the bound of the feature maps and volume features (None = the library default, 4094): the exponents of
    the activations' fp16 planes follow the bound MEASURED per frame (``fit``: ufr_frame_prepare measures, ufr_weights_fit_frame
    re-derives the table when a frame exceeds what it serves), so no side information about a checkpoint's feature scale
    is needed.  Weights of any finite magnitude pack without further ado."""

    def __init__(self, params: Dict[str, torch.Tensor], precision: Optional[int] = None,
                 input_abs_max: Optional[float] = None):
        lib = _lib.load()
        self.precision = precision
        self.input_abs_max = input_abs_max
        self._keep = []
        ptrs = []
        for key, shape in zip(RAW_WEIGHT_KEYS, RAW_WEIGHT_SHAPES):
            if key not in params:
                raise UfrError(f"missing parameter {key}")
            t = params[key].detach()
            if tuple(t.shape) != tuple(shape):
                raise UfrError(f"{key}: shape {tuple(t.shape)}, expected {tuple(shape)}")
            t = t.contiguous()
            ptrs.append(_dev(t, key))
            self._keep.append(t)
        self.raw = _lib.RawWeights()
        C.memmove(C.byref(self.raw), (C.c_void_p * 40)(*ptrs), C.sizeof(self.raw))
        self.device = self._keep[0].device
        self.packed = torch.empty(lib.ufr_packed_weights_bytes() // 4, dtype=torch.float32, device=self.device)
        self.serial = next(_PACK_SERIAL)
        self.epoch = 0          # bumped by every pack: a frame is fitted once per (frame, epoch)
        self.repack(check=True)

    def repack(self, check: bool = False) -> None:
        """Call after the parameters changed in place (e.g. an optimizer step): the planes AND their exponents follow
        the parameters.  Asynchronous: a non-finite parameter raises the sticky status, which the next compute call (or
        ``status_poll``) reports; ``check=True`` synchronises and raises at once (construction does)."""
        lib = _lib.load()
        if self.input_abs_max is None:
            rc = lib.ufr_weights_pack(C.byref(self.raw), self.packed.data_ptr(), _stream())
        else:
            rc = lib.ufr_weights_pack_for(C.byref(self.raw), self.packed.data_ptr(), float(self.input_abs_max), _stream())
        _lib.check(rc, "ufr_weights_pack")
        self.epoch += 1
        if check:
            status_poll(True, mask=4)    # the pack's own bit: an unrelated, still unreported overflow must not fail a valid pack

    def fit(self, frame: "FrameHandle") -> None:
        """The activation exponents follow ``frame``'s measured feature bound (ufr_weights_fit_frame): one tiny asynchronous
        kernel, issued once per (frame, pack) -- a no-op on the device unless the frame exceeds the bound the table serves."""
        key = (self.serial, self.epoch)       # a process-wide serial number, not id(self): an id is reused after collection
        if key in frame._fitted:
            return
        _lib.check(_lib.load().ufr_weights_fit_frame(self.packed.data_ptr(), C.byref(frame.frame), _stream()), "ufr_weights_fit_frame")
        if len(frame._fitted) > 8:
            frame._fitted.clear()
        frame._fitted.add(key)

    def mode(self) -> int:
        return resolve_precision(self.precision)

    def scale_exponents(self) -> Dict[str, tuple]:
        """(s_M, a_M) per dense matrix, read back from the packed blob's scale table (synchronises; for tests and reports)."""
        import math
        lib = _lib.load()
        off, n = lib.ufr_packed_scale_table_offset(), lib.ufr_packed_scale_table_entries()
        t = self.packed[off:off + 4 * n].cpu().view(n, 4)
        names = ("vt_q", "vt_k", "vt_v", "vt_merge", "vt_mlp0", "vt_mlp2", "rt_q", "rt_k", "rt_v", "rt_merge", "rt_mlp0",
                 "rt_mlp2", "dm0", "dm2", "dm4", "rw0", "rw2", "rw4")
        return {nm: (int(round(math.log2(float(t[i, 3])))), int(round(math.log2(float(t[i, 0]))))) for i, nm in enumerate(names)}

    @property
    def variance(self) -> torch.Tensor:
        return self._keep[-1]


class FrameHandle:
    """Per-frame channel-last copies + camera constants (ufr_frame_prepare)."""

    def __init__(self, batch: dict, source_imgs_feat: torch.Tensor, feature_volume: Optional[dict], match_feature,
                 stages=("stage1", "stage2", "stage3")):
        """``feature_volume`` / ``match_feature`` may be None: such a handle only serves ``project_gather`` calls that
        pass ``vol24_in`` / ``sim8_in`` (RayTransformer.forward gets them as arguments)."""
        lib = _lib.load()
        imgs = batch["source_imgs"]
        if imgs.shape[0] != 1:
            raise UfrError("the per-ray path handles one frame per call (B=1), as the reference's test loop does")
        _, NV, _, H, W = imgs.shape
        s_idx = batch["start_idx"] if "start_idx" in batch else 1  # model.py:313
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        self._keep = dict(
            imgs=f32(imgs[0]), depth=f32(batch["depth_info"][0]), feat=f32(source_imgs_feat[0]),
        )
        if match_feature is not None:
            self._keep["match"] = f32(match_feature[0][0])
        if tuple(self._keep["depth"].shape) != (NV, H, W):
            # (1, B*V, H, W) of a B > 1 batch handed over whole would silently render every frame with frame 0's maps
            raise UfrError(f"depth_info shape {tuple(batch['depth_info'].shape)}: expected (1, {NV}, {H}, {W})")
        d = _lib.FrameDesc()
        d.NV, d.H, d.W = NV, H, W
        d.source_imgs = _dev(self._keep["imgs"], "source_imgs")
        d.depth_info = _dev(self._keep["depth"], "depth_info")
        d.feat = _dev(self._keep["feat"], "source_imgs_feat")
        if tuple(self._keep["feat"].shape) != (NV, 32, H // 4, W // 4):
            raise UfrError(f"source_imgs_feat shape {tuple(source_imgs_feat.shape)}")
        if match_feature is not None:
            d.match = _dev(self._keep["match"], "match_feature")
            if tuple(self._keep["match"].shape) != (NV, 32 * (NV - 1), H // 4, W // 4):
                raise UfrError(f"match_feature shape {tuple(match_feature[0].shape)}")
        for i, st in enumerate(stages if feature_volume is not None else ()):
            fv = f32(feature_volume[st]["feature_volume"])
            wv = f32(feature_volume[st]["weight_volume"])
            if fv.shape[0] != NV or fv.shape[1] != 8 or wv.shape[1] != 1 or fv.shape[2:] != wv.shape[2:]:
                raise UfrError(f"{st}: volume shapes {tuple(fv.shape)} / {tuple(wv.shape)}")
            self._keep[f"fv{i}"], self._keep[f"wv{i}"] = fv, wv
            d.vol_feat[i], d.vol_weight[i] = _dev(fv, st), _dev(wv, st)
            d.vol_D[i], d.vol_H[i], d.vol_W[i] = fv.shape[2], fv.shape[3], fv.shape[4]
        # small camera constants: host copies
        host = lambda t: t.detach().to("cpu", torch.float32).contiguous()
        self._host = dict(
            poses=host(batch["source_poses"][0]),
            cam_pos=host(batch["source_poses_inv"][0, :, :3, 3]),
            ref_pos=host(batch["ref_pose_inv"][0, :3, 3]),
            w2c_z=host(batch["w2cs"][0, s_idx:, 2, :]),
        )
        if self._host["w2c_z"].shape[0] != NV:
            raise UfrError("w2cs[s_idx:] does not match the number of source views")
        fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))
        d.source_poses, d.source_cam_pos = fp(self._host["poses"]), fp(self._host["cam_pos"])
        d.ref_cam_pos, d.w2c_row2 = fp(self._host["ref_pos"]), fp(self._host["w2c_z"])
        if "near_fars" in batch:
            nf = batch["near_fars"][0][0].detach().cpu()
            d.vol_near, d.vol_far = float(nf[0]), float(nf[1])
        elif feature_volume is not None:
            raise UfrError("batch['near_fars'] is required to look up the frustums (model.py:328)")
        nbytes = lib.ufr_frame_workspace_bytes(C.byref(d))
        if nbytes == 0:
            raise UfrError("frame: " + lib.ufr_last_error().decode())
        self.device = self._keep["imgs"].device
        self.workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self.frame = _lib.Frame()
        _lib.check(lib.ufr_frame_prepare(C.byref(d), self.workspace.data_ptr(), nbytes, C.byref(self.frame), _stream()),
                   "ufr_frame_prepare")
        self.NV, self.H, self.W = NV, H, W
        self._fitted = set()    # (id(PackedWeights), its pack epoch) this frame's feature bound was handed to
        self.near_z, self.far_z = float(d.vol_near), float(d.vol_far)
        # view-dependent state of the whole-frame renderer (absent when the handle only serves RayTransformer.forward)
        self.ray_o = [float(v) for v in batch["ray_o"][0].detach().cpu()] if "ray_o" in batch else None
        self.ray_d = f32(batch["ray_d"][0]) if "ray_d" in batch else None
        self.cam_ray_d = f32(batch["cam_ray_d"][0]) if "cam_ray_d" in batch else None


# ----------------------------------------------------------------------------- per-op wrappers
def sample_fixed(near: torch.Tensor, far: torch.Tensor, U: torch.Tensor) -> torch.Tensor:
    SN, RN = U.shape
    z = torch.empty(RN, SN, dtype=torch.float32, device=U.device)
    _lib.check(_lib.load().ufr_sample_fixed(_dev(near, "near"), _dev(far, "far"), _dev(U, "U"), z.data_ptr(), RN, SN,
                                            _stream()), "ufr_sample_fixed")
    return z


def sample_importance_merge(weight: torch.Tensor, z: torch.Tensor, U2: torch.Tensor, want_fine: bool = True):
    RN, SN = z.shape
    PN = U2.shape[0]
    z_fine = torch.empty(RN, PN, dtype=torch.float32, device=z.device) if want_fine else None
    z_all = torch.empty(RN, SN + PN, dtype=torch.float32, device=z.device)
    _lib.check(_lib.load().ufr_sample_importance_merge(
        _dev(weight, "weight"), _dev(z, "z"), _dev(U2, "U2"), _opt(z_fine, "z_fine"), z_all.data_ptr(), RN, SN, PN,
        _stream()), "ufr_sample_importance_merge")
    return z_fine, z_all


def points(ray_o: torch.Tensor, ray_d: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    RN, SN = z.shape
    stride = 0 if ray_o.numel() == 3 else 3
    out = torch.empty(RN, SN, 3, dtype=torch.float32, device=z.device)
    _lib.check(_lib.load().ufr_points(_dev(ray_o, "ray_o"), stride, _dev(ray_d, "ray_d"), _dev(z, "z"), out.data_ptr(),
                                      RN, SN, _stream()), "ufr_points")
    return out


def project_gather(frame: FrameHandle, weights: PackedWeights, ray_o: torch.Tensor, ray_d: torch.Tensor,
                   z: torch.Tensor, debug: bool = False, want_sim8: bool = False, want_xy: bool = False,
                   vol24_in: Optional[torch.Tensor] = None, sim8_in: Optional[torch.Tensor] = None,
                   sim8_out: Optional[torch.Tensor] = None, out=None):
    """``out`` = (x (P,NV,80), rgb (P,NV,4), dirs (P,NV,4)): write into these (row ranges of the two-pass step's pool)."""
    RN, SN = z.shape
    P, NV, dev = RN * SN, frame.NV, z.device
    if out is not None:
        x, rgb, dirs = out
        assert x.shape == (P, NV, _lib.TOKEN_DIM) and rgb.shape == (P, NV, 4) and dirs.shape == (P, NV, 4)
        assert x.is_contiguous() and rgb.is_contiguous() and dirs.is_contiguous()
    else:
        x = torch.empty(P, NV, _lib.TOKEN_DIM, dtype=torch.float32, device=dev)
        rgb = torch.empty(P, NV, 4, dtype=torch.float32, device=dev)
        dirs = torch.empty(P, NV, 4, dtype=torch.float32, device=dev)
    dbg = {}
    if debug:       # NaN-filled: a row the kernel leaves unwritten must not pass by holding an earlier call's values
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        dbg = dict(sim8=nan(P, 8), vol24=nan(P, 24), xy=nan(NV, P, 2), mask_z=nan(NV, P))
    else:
        if sim8_out is not None:   # ... into a row range of the two-pass step's pool
            dbg["sim8"] = sim8_out
        elif want_sim8:   # the backward of pre_sim_mlp needs its input
            dbg["sim8"] = torch.empty(P, 8, device=dev)
        if want_xy:     # points_in_pixel of the reference's return tuples
            dbg["xy"] = torch.empty(NV, P, 2, device=dev)
    stride = 0 if ray_o.numel() == 3 else 3
    weights.fit(frame)      # the tokens gathered here meet `weights`' dense layers next: their exponents follow this frame
    _lib.check(_lib.load().ufr_project_gather(
        C.byref(frame.frame), C.byref(weights.raw), _dev(ray_o, "ray_o"), stride, _dev(ray_d, "ray_d"), _dev(z, "z"),
        RN, SN, x.data_ptr(), rgb.data_ptr(), dirs.data_ptr(), _opt(dbg.get("sim8"), "sim8"),
        _opt(dbg.get("vol24"), "vol24"), _opt(dbg.get("xy"), "xy"), _opt(dbg.get("mask_z"), "mask_z"),
        _opt(vol24_in, "vol24_in"), _opt(sim8_in, "sim8_in"), _stream()),
        "ufr_project_gather")
    return x, rgb, dirs, dbg


def _max_points(NV: int) -> int:
    """points one transformer launch addresses (32-bit offsets: P * (NV + 1) * 80 < 2^30, include/ufr.h)"""
    return ((1 << 30) - 1) // ((NV + 1) * _lib.TOKEN_DIM)


def aggregate(weights: PackedWeights, x: torch.Tensor, rgb: torch.Tensor, dirs: torch.Tensor, RN: int, SN: int,
              debug: bool = False, keep_workspace: bool = False, precision: Optional[int] = None):
    lib = _lib.load()
    NV, dev = x.shape[1], x.device
    P = RN * SN
    rays_max = _max_points(NV) // SN
    if RN > rays_max >= 1:      # beyond one launch's 32-bit addressing: rays are independent, so call per ray range
        parts = [aggregate(weights, x[r0 * SN:(r0 + rays_max) * SN], rgb[r0 * SN:(r0 + rays_max) * SN],
                           dirs[r0 * SN:(r0 + rays_max) * SN], min(rays_max, RN - r0), SN, debug, keep_workspace, precision)
                 for r0 in range(0, RN, rays_max)]
        dbg = {k: torch.cat([p[2][k] for p in parts]) for k in parts[0][2]}
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), dbg
    radiance = torch.empty(P, 3, dtype=torch.float32, device=dev)
    srdf = torch.empty(RN, SN, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.ufr_aggregate_workspace_bytes(RN, SN, NV) // 4, dtype=torch.float32, device=dev)
    dbg = {}
    if debug:
        dbg = dict(view_out=torch.empty(P, NV + 1, _lib.TOKEN_DIM, device=dev), ray_out=torch.empty(P, _lib.RAY_DIM, device=dev))
    _lib.check(lib.ufr_aggregate(weights.packed.data_ptr(), _dev(x, "x_tokens"), _dev(rgb, "rgb"), _dev(dirs, "dir"),
                                 RN, SN, NV, radiance.data_ptr(), srdf.data_ptr(), ws.data_ptr(),
                                 _opt(dbg.get("view_out"), "view_out"), _opt(dbg.get("ray_out"), "ray_out"),
                                 weights.mode() if precision is None else precision, _stream()),
               "ufr_aggregate")
    if keep_workspace:   # the head of the workspace is the view transformer's token-0 output (P,80): the backward needs it
        dbg["token0"] = ws[: P * _lib.TOKEN_DIM].view(P, _lib.TOKEN_DIM)
    return radiance, srdf, dbg


def composite(z: torch.Tensor, radiance: torch.Tensor, srdf: torch.Tensor, variance: torch.Tensor,
              row: Optional[torch.Tensor] = None):
    """``row`` (RN,SN) int32: slot (ray, s) takes its colour from ``radiance.view(-1, 3)[row]`` (the sample pool)."""
    RN, SN = z.shape
    dev = z.device
    rgb = torch.empty(RN, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(RN, dtype=torch.float32, device=dev)
    opacity = torch.empty(RN, dtype=torch.float32, device=dev)
    weight = torch.empty(RN, SN, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ufr_composite(_dev(z, "z"), _dev(radiance, "radiance"),
                                         None if row is None else _dev(row, "row", torch.int32), _dev(srdf, "srdf"),
                                         _dev(variance, "variance"), RN, SN, rgb.data_ptr(), depth.data_ptr(),
                                         opacity.data_ptr(), weight.data_ptr(), _stream()), "ufr_composite")
    return rgb, depth, opacity, weight


# ----------------------------------------------------------------------------- backward (training step)
class GradBuffer:
    """One flat fp32 buffer holding the gradients of the 40 per-ray parameters in RAW_WEIGHT_KEYS order (the kernels
    accumulate into it with atomics; one buffer = one all-reduce for data-parallel training)."""

    def __init__(self, device):
        sizes = [max(1, int(torch.Size(s).numel())) for s in RAW_WEIGHT_SHAPES]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + (n + 3) // 4 * 4)        # 16-byte aligned slots
        self.flat = torch.zeros(offs[-1], dtype=torch.float32, device=device)
        self.views = {k: self.flat[o:o + n].view(shape) for k, shape, o, n in zip(RAW_WEIGHT_KEYS, RAW_WEIGHT_SHAPES, offs, sizes)}
        self.raw = _lib.RawGrads()
        for i, o in enumerate(offs[:-1]):
            self.raw.p[i] = self.flat.data_ptr() + 4 * o

    def grad(self, key: str) -> torch.Tensor:
        return self.views[key]


def composite_bwd(z, radiance, srdf, variance, d_rgb, d_depth, d_opacity, d_weight, row=None, d_radiance=None,
                  accumulate: bool = False, d_variance=None):
    """``row`` / ``d_radiance`` / ``accumulate``: the pool form -- d_radiance rows are those ``row`` names inside the given
    pool-sized buffer, added to its content when ``accumulate``.  ``d_variance`` (a zeroed scalar) is accumulated."""
    RN, SN = z.shape
    dev = z.device
    if d_radiance is None:
        d_radiance = torch.empty(RN, SN, 3, dtype=torch.float32, device=dev)
    d_srdf = torch.empty(RN, SN, dtype=torch.float32, device=dev)
    if d_variance is None:
        d_variance = torch.zeros((), dtype=torch.float32, device=dev)
    keep = []

    def opt(t, n):
        if t is None:
            return None
        keep.append(t.contiguous())
        return _dev(keep[-1], n)

    _lib.check(_lib.load().ufr_composite_bwd(
        _dev(z, "z"), _dev(radiance, "radiance"), None if row is None else _dev(row, "row", torch.int32), _dev(srdf, "srdf"),
        _dev(variance, "variance"), RN, SN,
        opt(d_rgb, "d_rgb"), opt(d_depth, "d_depth"), opt(d_opacity, "d_opacity"), opt(d_weight, "d_weight"),
        _dev(d_radiance, "d_radiance"), int(accumulate), d_srdf.data_ptr(), _dev(d_variance, "d_variance"), _stream()),
        "ufr_composite_bwd")
    return d_radiance, d_srdf, d_variance


def render_loss(rgb, depth, rgb2, depth2, rgb_gt, depth_gt, near_fars, weight_rgb: float = 1.0, weight_depth: float = 1.0):
    """ufr_render_loss (code1/model.py:552-566): both passes' colours (B,RN,3) / ray depths (B,RN), the ground truth of the
    same shapes, ``near_fars`` = batch['near_fars'] (B,V,2).  -> ``loss (5,)`` = [total, rgb coarse, rgb fine, depth coarse,
    depth fine] and the cotangents ``d_rgb, d_depth, d_rgb2, d_depth2`` of the total, shaped as the inputs."""
    B, RN = depth_gt.shape
    dev = depth_gt.device
    c = lambda t: t.detach().float().contiguous()
    rgb, depth, rgb2, depth2, rgb_gt, depth_gt, nf = c(rgb), c(depth), c(rgb2), c(depth2), c(rgb_gt), c(depth_gt), c(near_fars)
    if tuple(rgb.shape) != (B, RN, 3) or tuple(rgb2.shape) != (B, RN, 3) or tuple(rgb_gt.shape) != (B, RN, 3) or \
            tuple(depth.shape) != (B, RN) or tuple(depth2.shape) != (B, RN) or nf.shape[0] != B or nf.shape[-1] != 2:
        raise UfrError(f"render_loss: shapes {tuple(rgb.shape)} {tuple(depth.shape)} {tuple(rgb2.shape)} {tuple(depth2.shape)} "
                            f"{tuple(rgb_gt.shape)} {tuple(depth_gt.shape)} {tuple(nf.shape)}")
    out = torch.empty(5 + 8 * B * RN, dtype=torch.float32, device=dev)       # one allocation: loss | d_rgb | d_depth | d_rgb2 | d_depth2
    n = B * RN
    loss, d_rgb, d_depth, d_rgb2, d_depth2 = out[:5], out[5:5 + 3 * n], out[5 + 3 * n:5 + 4 * n], out[5 + 4 * n:5 + 7 * n], out[5 + 7 * n:]
    _lib.check(_lib.load().ufr_render_loss(
        _dev(rgb, "rgb"), _dev(depth, "depth"), _dev(rgb2, "rgb2"), _dev(depth2, "depth2"), _dev(rgb_gt, "rgb_gt"),
        _dev(depth_gt, "depth_gt"), _dev(nf, "near_fars"), nf[0].numel(), B, RN, float(weight_rgb), float(weight_depth),
        loss.data_ptr(), d_rgb.data_ptr(), d_depth.data_ptr(), d_rgb2.data_ptr(), d_depth2.data_ptr(), _stream()), "ufr_render_loss")
    return loss, d_rgb.view(B, RN, 3), d_depth.view(B, RN), d_rgb2.view(B, RN, 3), d_depth2.view(B, RN)


def aggregate_bwd(weights: PackedWeights, grads: GradBuffer, x, rgb, dirs, token0, RN: int, SN: int, d_radiance, d_srdf,
                  precision: Optional[int] = None):
    """-> (d_pv (P,40), {}) -- the empty dict keeps the call sites of the former debug dump (gone with ABI 500)."""
    lib = _lib.load()
    NV, dev = x.shape[1], x.device
    P = RN * SN
    d_pv = torch.empty(P, 40, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.ufr_aggregate_bwd_workspace_bytes(RN, SN, NV) // 4, dtype=torch.float32, device=dev)
    _lib.check(lib.ufr_aggregate_bwd(
        C.byref(weights.raw), C.byref(grads.raw), weights.packed.data_ptr(), _dev(x, "x_tokens"), _dev(rgb, "rgb"),
        _dev(dirs, "dir"), _dev(token0, "token0"), RN, SN, NV, _dev(d_radiance.contiguous(), "d_radiance"),
        _dev(d_srdf.contiguous(), "d_srdf"), d_pv.data_ptr(), ws.data_ptr(),
        weights.mode() if precision is None else precision, _stream()),
        "ufr_aggregate_bwd")
    return d_pv, {}


def project_gather_bwd_workspace_floats(frame: FrameHandle) -> int:
    return _lib.load().ufr_project_gather_bwd_workspace_bytes(C.byref(frame.frame)) // 4


def project_gather_bwd(frame: FrameHandle, weights: PackedWeights, grads: GradBuffer, ray_o, ray_d, z, sim8, d_pv,
                       grad_vol_feat, grad_vol_weight, precision: Optional[int] = None,
                       row: Optional[torch.Tensor] = None, accumulate: bool = True,
                       zeroed_workspace: Optional[torch.Tensor] = None, presim: bool = True) -> None:
    """Writes the frustum gradients grad_vol_feat[s] (NV,8,D,Hs,Ws) / grad_vol_weight[s] (NV,1,D,Hs,Ws) -- added to what the
    tensors hold (``accumulate``, the default: pass zeros) or overwriting them whole (``accumulate=False``: pass
    ``torch.empty``, no zero-fill needed) -- and accumulates the pre_sim_mlp gradients into `grads`.  ``row`` (RN,SN) int32:
    ``sim8`` / ``d_pv`` are pool tensors and slot (ray, s) owns ``d_pv[row[ray, s]]``.  ``zeroed_workspace``: the scatter's
    record volume (project_gather_bwd_workspace_floats), already zero-filled by the caller -- ordered before this call.
    ``presim=False``: the volume scatter only (UFR_GBWD_NO_PRESIM); the pre_sim_mlp half is the call with both lists None."""
    RN, SN = z.shape
    lib = _lib.load()
    stride = 0 if ray_o.numel() == 3 else 3
    gf = gw = ws = None        # both None: pre_sim_mlp gradients only
    if grad_vol_feat is not None:
        gf = (C.c_void_p * 3)(*[_dev(t, "grad_vol_feat") for t in grad_vol_feat])
        gw = (C.c_void_p * 3)(*[_dev(t, "grad_vol_weight") for t in grad_vol_weight])
        # channel-last record volume of the scatter (zeroed by the library unless the caller did)
        ws = zeroed_workspace if zeroed_workspace is not None else torch.empty(
            project_gather_bwd_workspace_floats(frame), dtype=torch.float32, device=z.device)
    _lib.check(lib.ufr_project_gather_bwd(
        C.byref(frame.frame), C.byref(weights.raw), C.byref(grads.raw), _dev(ray_o, "ray_o"), stride, _dev(ray_d, "ray_d"),
        _dev(z, "z"), RN, SN, _dev(sim8, "sim8"), _dev(d_pv, "d_pv"), None if row is None else _dev(row, "row", torch.int32),
        gf, gw, int(bool(accumulate)) | (2 if (zeroed_workspace is not None and ws is not None) else 0) | (0 if presim else 4),
        None if ws is None else ws.data_ptr(),
        weights.mode() if precision is None else precision, _stream()), "ufr_project_gather_bwd")


# ----------------------------------------------------------------------------- halves of aggregate / sample pool
def sample_importance_pool(weight: torch.Tensor, z: torch.Tensor, U2: torch.Tensor):
    """-> z_all (RN,SN+PN) sorted, z_new (RN,PN) sorted along the ray, row (RN,SN+PN) int32: pool row of every merged slot
    (pool = [RN*SN coarse rows | RN*PN new rows])."""
    RN, SN = z.shape
    PN = U2.shape[0]
    dev = z.device
    z_all = torch.empty(RN, SN + PN, dtype=torch.float32, device=dev)
    z_new = torch.empty(RN, PN, dtype=torch.float32, device=dev)
    row = torch.empty(RN, SN + PN, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().ufr_sample_importance_pool(_dev(weight, "weight"), _dev(z, "z"), _dev(U2, "U2"), z_all.data_ptr(),
                                                      z_new.data_ptr(), row.data_ptr(), RN, SN, PN, _stream()),
               "ufr_sample_importance_pool")
    return z_all, z_new, row


def view_transform(weights: PackedWeights, x: torch.Tensor, rgb: torch.Tensor, dirs: torch.Tensor,
                   token0: Optional[torch.Tensor] = None, radiance: Optional[torch.Tensor] = None,
                   precision: Optional[int] = None):
    """``token0`` (P,80) / ``radiance`` (P,3): optional destinations (row ranges of the two-pass step's sample pool)."""
    P, NV = x.shape[0], x.shape[1]
    if token0 is None:
        token0 = torch.empty(P, _lib.TOKEN_DIM, dtype=torch.float32, device=x.device)
    if radiance is None:
        radiance = torch.empty(P, 3, dtype=torch.float32, device=x.device)
    if token0.shape[0] != P or radiance.shape[0] != P:
        raise UfrError("view_transform: destination rows do not match the number of points")
    pmax = _max_points(NV)
    if P > pmax:                # beyond one launch's 32-bit addressing: points are independent, so call per point range
        for p0 in range(0, P, pmax):
            view_transform(weights, x[p0:p0 + pmax], rgb[p0:p0 + pmax], dirs[p0:p0 + pmax], token0[p0:p0 + pmax],
                           radiance[p0:p0 + pmax], precision)
        return token0, radiance
    _lib.check(_lib.load().ufr_view_transform(weights.packed.data_ptr(), _dev(x, "x_tokens"), _dev(rgb, "rgb"), _dev(dirs, "dir"),
                                              P, NV, _dev(token0, "token0"), _dev(radiance, "radiance"),
                                              weights.mode() if precision is None else precision, _stream()),
               "ufr_view_transform")
    return token0, radiance


def ray_transform(weights: PackedWeights, token0: torch.Tensor, RN: int, SN: int, row: Optional[torch.Tensor] = None,
                  precision: Optional[int] = None) -> torch.Tensor:
    """``row`` (RN,SN) int32: slot (ray, s) reads ``token0[row]`` (the sample pool); None = slot order."""
    lib = _lib.load()
    srdf = torch.empty(RN, SN, dtype=torch.float32, device=token0.device)
    ws = torch.empty(lib.ufr_ray_transform_workspace_bytes(SN) // 4, dtype=torch.float32, device=token0.device)
    _lib.check(lib.ufr_ray_transform(weights.packed.data_ptr(), _dev(token0, "token0"),
                                     None if row is None else _dev(row, "row", torch.int32), RN, SN, srdf.data_ptr(),
                                     ws.data_ptr(), weights.mode() if precision is None else precision, _stream()),
               "ufr_ray_transform")
    return srdf


def view_tape_block_points(NV: int) -> int:
    return int(_lib.load().ufr_view_tape_block_points(NV))


def view_transform_tape(weights: PackedWeights, x, rgb, dirs, token0, radiance, workspace: torch.Tensor, p0: int, P_total: int,
                        precision: Optional[int] = None) -> None:
    """Training forward of the view transformer for the pool rows [p0, p0 + P): writes ``token0`` / ``radiance`` (the
    range's rows) like view_transform and records the tape into ``workspace`` (view_transform_bwd_workspace(P_total, NV)),
    whose backward then runs with ``stages=STAGE_DGRAD | STAGE_WGRAD``."""
    P, NV = x.shape[0], x.shape[1]
    _lib.check(_lib.load().ufr_view_transform_tape(
        weights.packed.data_ptr(), _dev(x, "x_tokens"), _dev(rgb, "rgb"), _dev(dirs, "dir"), P, NV, _dev(token0, "token0"),
        _dev(radiance, "radiance"), workspace.data_ptr(), p0, P_total, weights.mode() if precision is None else precision,
        _stream()), "ufr_view_transform_tape")


def ray_transform_tape(weights: PackedWeights, token0: torch.Tensor, RN: int, SN: int, workspace: torch.Tensor,
                       row: Optional[torch.Tensor] = None, precision: Optional[int] = None) -> torch.Tensor:
    """Training forward of the ray transformer: srdf like ray_transform, the tape into ``workspace``
    (ray_transform_bwd_workspace(RN, SN)); its backward then runs without STAGE_TAPE."""
    srdf = torch.empty(RN, SN, dtype=torch.float32, device=token0.device)
    _lib.check(_lib.load().ufr_ray_transform_tape(
        weights.packed.data_ptr(), _dev(token0, "token0"), None if row is None else _dev(row, "row", torch.int32), RN, SN,
        srdf.data_ptr(), workspace.data_ptr(), weights.mode() if precision is None else precision, _stream()),
        "ufr_ray_transform_tape")
    return srdf


def ray_transform_bwd_workspace(RN: int, SN: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().ufr_ray_transform_bwd_workspace_bytes(RN, SN) // 4, dtype=torch.float32, device=device)


def ray_transform_bwd(weights: PackedWeights, grads: GradBuffer, token0: torch.Tensor, RN: int, SN: int, d_srdf: torch.Tensor,
                      row: Optional[torch.Tensor] = None, out=None, accumulate: bool = False, precision: Optional[int] = None,
                      _workspace_out: Optional[list] = None, stages: int = 7, workspace: Optional[torch.Tensor] = None):
    """-> the two partial d token0 buffers of the ray kernel's sweeps (their sum is the gradient).  Plain form: (RN*SN,80)
    in slot order.  Pool form: ``row`` maps slots to rows of ``token0`` and of the two pool-sized buffers ``out=(a, b)``,
    which are overwritten or, with ``accumulate``, added to.  ``b`` may be None: nothing is zero-filled then (the caller owns
    the second buffer, e.g. lets another pass write it concurrently)."""
    lib = _lib.load()
    dev = token0.device
    if out is None:
        a = torch.empty(RN * SN, _lib.TOKEN_DIM, dtype=torch.float32, device=dev)
        b = torch.empty(RN * SN, _lib.TOKEN_DIM, dtype=torch.float32, device=dev)
    else:
        a, b = out
    ws = workspace if workspace is not None else ray_transform_bwd_workspace(RN, SN, dev)
    d_srdf = d_srdf.contiguous()
    # stages (include/ufr.h: ufr_ray_transform_bwd_stages): tape + data gradients (3) write ``out``; the weight gradients (4)
    # feed nothing downstream -- a caller may run them later / elsewhere on the same ``workspace``
    _lib.check(lib.ufr_ray_transform_bwd_stages(C.byref(weights.raw), C.byref(grads.raw), weights.packed.data_ptr(),
                                                _dev(token0, "token0"), None if row is None else _dev(row, "row", torch.int32),
                                                RN, SN, _dev(d_srdf, "d_srdf"), _dev(a, "d_token0_a"), _opt(b, "d_token0_b"),
                                                int(accumulate), ws.data_ptr(), stages,
                                                weights.mode() if precision is None else precision, _stream()),
               "ufr_ray_transform_bwd")
    if _workspace_out is not None:      # development: the tape / cotangent tiles (tools/dev/ray_bwd_check.py)
        _workspace_out.append(ws)
    return a, b


STAGE_TAPE, STAGE_DGRAD, STAGE_WGRAD, STAGE_ALL = 1, 2, 4, 7


def view_transform_bwd_workspace(P: int, NV: int, device) -> torch.Tensor:
    """The tile buffers of the view transformer's backward (csrc/bwd_tape.h): pass the same tensor to every stage."""
    return torch.empty(_lib.load().ufr_view_transform_bwd_workspace_bytes(P, NV) // 4, dtype=torch.float32, device=device)


def view_transform_bwd(weights: PackedWeights, grads: GradBuffer, x, rgb, dirs, d_token0_a, d_token0_b, d_radiance,
                       precision: Optional[int] = None, d_pv: Optional[torch.Tensor] = None, stages: int = STAGE_ALL,
                       workspace: Optional[torch.Tensor] = None):
    """``stages`` (include/ufr.h: ufr_view_transform_bwd_stages): STAGE_TAPE needs only x / rgb / dirs, STAGE_DGRAD the
    cotangents (writes d_pv), STAGE_WGRAD nothing but the workspace -- a caller that splits them passes ONE ``workspace``
    (view_transform_bwd_workspace) to all and orders them with stream events."""
    P, NV = x.shape[0], x.shape[1]
    if d_pv is None and (stages & STAGE_DGRAD):
        d_pv = torch.empty(P, 40, dtype=torch.float32, device=x.device)
    ta = None if d_token0_a is None else d_token0_a.contiguous()
    tb = None if d_token0_b is None else d_token0_b.contiguous()
    dr = None if d_radiance is None else d_radiance.contiguous()
    lib = _lib.load()
    ws = workspace if workspace is not None else view_transform_bwd_workspace(P, NV, x.device)
    _lib.check(lib.ufr_view_transform_bwd_stages(
        C.byref(weights.raw), C.byref(grads.raw), weights.packed.data_ptr(), _dev(x, "x_tokens"), _dev(rgb, "rgb"),
        _dev(dirs, "dir"), _opt(ta, "d_token0_a"), _opt(tb, "d_token0_b"), _opt(dr, "d_radiance"), P, NV, _opt(d_pv, "d_pv"),
        ws.data_ptr(), stages, weights.mode() if precision is None else precision, _stream()), "ufr_view_transform_bwd")
    return d_pv


class RenderWorkspace:
    """Reusable scratch of ufr_render_rays (sized for `chunk_rays`)."""

    def __init__(self, device, SN: int, PN: int, NV: int, chunk_rays: int = 0, n_streams: int = 3):
        lib = _lib.load()
        self.chunk = chunk_rays if chunk_rays > 0 else lib.ufr_default_chunk_rays()
        self.n_streams = max(1, int(n_streams))
        self.key = (SN, PN, NV, self.chunk)
        self.nbytes = lib.ufr_render_workspace_bytes(self.chunk, SN, PN, NV) * self.n_streams
        self.buf = torch.empty(self.nbytes // 4, dtype=torch.float32, device=device)


def render_rays(frame: FrameHandle, weights: PackedWeights, ray_idx: torch.Tensor, U1: torch.Tensor,
                U2: Optional[torch.Tensor], coarse_only: bool = False, workspace: Optional[RenderWorkspace] = None,
                want_srdf: bool = True, out: Optional[dict] = None, pair: bool = False):
    """UFORecon.infer(extract_geometry=True) for the rays `ray_idx` (RN,) of the prepared frame.

    ``pair=True`` (ufr_render_rays_pair) also returns the coarse pass as ``rgb_coarse`` (RN,3) / ``depth_coarse`` (RN); on that
    route a frame without ``cam_ray_d`` renders as infer(extract_geometry=False) does (near/far as given; ``depth_z`` is None)."""
    if pair and coarse_only:
        raise UfrError("render_rays: pair=True returns both passes; coarse_only renders one")
    if frame.ray_d is None or frame.ray_o is None or (frame.cam_ray_d is None and not pair):
        raise UfrError("batch['ray_o'], ['ray_d'] and ['cam_ray_d'] are required for extract_geometry rendering")
    dev = frame.device
    RN = ray_idx.numel()
    SN = U1.shape[0]
    PN = 0 if coarse_only else U2.shape[0]
    S = SN + PN
    if workspace is None or workspace.key[:3] != (SN, PN, frame.NV):
        workspace = RenderWorkspace(dev, SN, PN, frame.NV)
    o = out or {}
    depth = o.get("depth", torch.empty(RN, dtype=torch.float32, device=dev))
    depth_z = o.get("depth_z", torch.empty(RN, dtype=torch.float32, device=dev)) if frame.cam_ray_d is not None else None
    rgb = o.get("rgb", torch.empty(RN, 3, dtype=torch.float32, device=dev))
    srdf = torch.empty(RN, S, dtype=torch.float32, device=dev) if want_srdf else None
    z_all = torch.empty(RN, S, dtype=torch.float32, device=dev) if want_srdf else None
    a = _lib.RenderArgs()
    a.frame = C.pointer(frame.frame)
    a.packed_weights = weights.packed.data_ptr()
    a.raw = C.pointer(weights.raw)
    a.ray_idx = _dev(ray_idx.reshape(-1), "ray_idx", torch.int64)
    a.ray_d, a.cam_ray_d = _dev(frame.ray_d, "ray_d"), _opt(frame.cam_ray_d, "cam_ray_d")
    a.ray_o = (C.c_float * 3)(*frame.ray_o)
    a.near_z, a.far_z = frame.near_z, frame.far_z
    a.U1 = _dev(U1, "U1")
    a.U2 = None if coarse_only else _dev(U2, "U2")
    if U1.shape[1] != RN or (not coarse_only and U2.shape[1] != RN):
        raise UfrError("U1/U2 must be (samples, RN)")
    a.RN, a.SN, a.PN, a.coarse_only = RN, SN, PN, int(coarse_only)
    a.precision = weights.mode()
    a.depth, a.depth_z, a.rgb = depth.data_ptr(), _opt(depth_z, "depth_z"), rgb.data_ptr()
    a.srdf = _opt(srdf, "srdf")
    a.z_all = _opt(z_all, "z_all")
    a.chunk_rays = workspace.chunk
    a.n_streams = workspace.n_streams
    a.workspace, a.workspace_bytes = workspace.buf.data_ptr(), workspace.nbytes
    if not pair:
        _lib.check(_lib.load().ufr_render_rays(C.byref(a), _stream()), "ufr_render_rays")
        return dict(depth=depth, depth_z=depth_z, rgb=rgb, srdf=srdf, z_all=z_all, workspace=workspace)
    rgb_coarse = o.get("rgb_coarse", torch.empty(RN, 3, dtype=torch.float32, device=dev))
    depth_coarse = o.get("depth_coarse", torch.empty(RN, dtype=torch.float32, device=dev))
    _lib.check(_lib.load().ufr_render_rays_pair(C.byref(a), _dev(rgb_coarse, "rgb_coarse"), _dev(depth_coarse, "depth_coarse"),
                                                _stream()), "ufr_render_rays_pair")
    return dict(depth=depth, depth_z=depth_z, rgb=rgb, srdf=srdf, z_all=z_all, workspace=workspace, rgb_coarse=rgb_coarse,
                depth_coarse=depth_coarse)


# ---- a validation frame's scores and previews (csrc/frame_metrics.hip; pipeline.validation_step is the caller)
FRAME_METRIC_KEYS = ("val/loss_rgb_coarse", "val/loss_rgb_fine", "psnr/coarse", "psnr/fine", "val/loss_depth_coarse",
                     "val/loss_depth_fine", "valid_pixels", "depth_coarse_max")


def frame_metrics(rgb_c: torch.Tensor, rgb_f: torch.Tensor, rgb_gt: torch.Tensor, depth_c: torch.Tensor, depth_f: torch.Tensor,
                  depth_gt: torch.Tensor, near: float, far: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ufr_frame_metrics: the eight float64 values of FRAME_METRIC_KEYS, on the device.  rgb_c / rgb_f (n,3), rgb_gt (3,n)
    planar (any trailing shape with n elements per channel, e.g. batch['ref_img'][0]), depths n values each.  Does not
    synchronise."""
    n = depth_c.numel()
    if n < 1 or rgb_c.numel() != 3 * n or rgb_f.numel() != 3 * n or rgb_gt.numel() != 3 * n or depth_f.numel() != n \
            or depth_gt.numel() != n or rgb_gt.shape[0] != 3 or rgb_c.shape[-1] != 3 or rgb_f.shape[-1] != 3:
        raise UfrError(f"frame_metrics: colours {tuple(rgb_c.shape)} {tuple(rgb_f.shape)} (n,3), ground truth {tuple(rgb_gt.shape)} "
                       f"(3,n), depths {tuple(depth_c.shape)} {tuple(depth_f.shape)} {tuple(depth_gt.shape)} (n)")
    lib = _lib.load()
    dev = depth_c.device
    out8 = torch.empty(8, dtype=torch.float64, device=dev) if out is None else out
    ws = torch.empty(lib.ufr_frame_metrics_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.ufr_frame_metrics(_dev(rgb_c, "rgb_c"), _dev(rgb_f, "rgb_f"), _dev(rgb_gt, "rgb_gt"), _dev(depth_c, "depth_c"),
                                     _dev(depth_f, "depth_f"), _dev(depth_gt, "depth_gt"), float(near), float(far), n,
                                     _dev(out8, "out8", torch.float64), ws.data_ptr(), _stream()), "ufr_frame_metrics")
    return out8


def frame_preview_u8(rgb: Optional[torch.Tensor], depth: Optional[torch.Tensor] = None, depth_max: Optional[torch.Tensor] = None,
                     depth_scale: float = 1.0):
    """ufr_frame_preview_u8: (rgb8 (n,3) uint8 = (rgb * 255).astype(uint8), depth8 (n) uint8 = ((depth * depth_scale) / (max *
    depth_scale) * 255).astype(uint8)) in numpy's float32 arithmetic; ``depth_max``: a one-element float64 CUDA tensor
    (frame_metrics(...)[7:8]).  Either half may be None.  Does not synchronise."""
    src = rgb if rgb is not None else depth
    if src is None:
        raise UfrError("frame_preview_u8: nothing to do (rgb and depth are both None)")
    n = src.numel() // 3 if rgb is not None else src.numel()
    if (rgb is not None and (rgb.shape[-1] != 3 or rgb.numel() != 3 * n)) or (depth is not None and depth.numel() != n) \
            or (depth is not None) != (depth_max is not None) or (depth_max is not None and depth_max.numel() != 1):
        raise UfrError("frame_preview_u8: rgb (n,3), depth (n) with a one-element depth_max")
    rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=src.device) if rgb is not None else None
    depth8 = torch.empty(n, dtype=torch.uint8, device=src.device) if depth is not None else None
    _lib.check(_lib.load().ufr_frame_preview_u8(
        _opt(rgb, "rgb"), _opt(depth, "depth"), None if depth_max is None else _dev(depth_max, "depth_max", torch.float64),
        float(depth_scale), n, None if rgb8 is None else rgb8.data_ptr(), None if depth8 is None else depth8.data_ptr(), _stream()),
        "ufr_frame_preview_u8")
    return rgb8, depth8


def fmt_layer(params, x: torch.Tensor, src: Optional[torch.Tensor]) -> torch.Tensor:
    """One FMT encoder layer on the GPU (ufr_fmt_layer).  ``params``: the 16 tensors in ufr_fmt_layer_weights order;
    x (N,T,32); src (N,S,32) or None for self-attention."""
    lib = _lib.load()
    N, T, D = x.shape
    if D != 32:
        raise UfrError(f"fmt_layer: d_model {D}, the kernel is built for 32")
    w = _lib.FmtLayerWeights()
    keep = []
    for name, t in zip([f[0] for f in _lib.FmtLayerWeights._fields_], params):
        t = t.detach().contiguous()
        keep.append(t)
        setattr(w, name, _dev(t, "fmt." + name))
    x = x.contiguous()
    S = T
    if src is not None:
        src = src.contiguous()
        if src.shape[0] != N or src.shape[2] != D:
            raise UfrError(f"fmt_layer: source tokens {tuple(src.shape)} do not match {tuple(x.shape)}")
        S = src.shape[1]
    out = torch.empty_like(x)
    ws = torch.empty(lib.ufr_fmt_layer_workspace_bytes(N, S) // 4, dtype=torch.float32, device=x.device)
    _lib.check(lib.ufr_fmt_layer(C.byref(w), _dev(x, "x"), _opt(src, "src"), N, T, S, out.data_ptr(), ws.data_ptr(),
                                 _stream()), "ufr_fmt_layer")
    return out


def set_matrix_precision(mode: int) -> None:
    """What PRECISION_DEFAULT resolves to (include/ufr.h): PRECISION_FP32 (the 1e-4 parity mode) or PRECISION_16BIT (one
    16-bit plane per operand: the mixed-precision training mode of BASELINE configs[4]).  A convenience for tools; a
    model pins its mode with ``UFORecon(args, precision=...)`` / ``PackedWeights(..., precision=...)``, and an autograd
    node always runs its backward in the mode its forward ran in."""
    _lib.check(_lib.load().ufr_set_matrix_precision(int(mode)), "ufr_set_matrix_precision")


def get_matrix_precision() -> int:
    return int(_lib.load().ufr_get_matrix_precision())


def profile_enable(on: bool) -> None:
    _lib.load().ufr_profile_enable(int(on))


def profile_read() -> dict:
    cap = 16
    names = (C.c_char_p * cap)()
    ms = (C.c_float * cap)()
    launches = (C.c_int32 * cap)()
    n = _lib.load().ufr_profile_read(names, ms, launches, cap)
    return {names[i].decode(): dict(ms=float(ms[i]), launches=int(launches[i])) for i in range(n)}


def marching_cubes(vol: torch.Tensor, level: float = 0.0):
    """Marching cubes on the device (ufr_marching_cubes_*): ``vol`` a CUDA fp32 contiguous (X,Y,Z) volume, z fastest (each
    dim >= 2).  Returns device tensors on the current stream: ``verts`` (V,3) fp32 in voxel-index coordinates, ``faces``
    (F,3) int32, ``normals`` (V,3) fp32 (+grad f, unit length), in the order include/ufr.h fixes.  One host
    synchronisation (the counts size the outputs).  A volume without a crossing of ``level`` gives empty (0,3) tensors
    (scikit-image raises there instead)."""
    if vol.dim() != 3:
        raise UfrError(f"marching_cubes: expected a 3-D volume, got shape {tuple(vol.shape)}")
    lib = _lib.load()
    dim = (C.c_int32 * 3)(*[int(d) for d in vol.shape])
    nbytes = lib.ufr_marching_cubes_workspace_bytes(dim)
    if nbytes == 0:
        raise UfrError(f"marching_cubes: volume {tuple(vol.shape)} unsupported (every dim >= 2, fewer than 2^31 voxels)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    counts = (C.c_int32 * 2)()
    p = _dev(vol, "vol")
    _lib.check(lib.ufr_marching_cubes_count(p, dim, float(level), ws.data_ptr(), nbytes, counts, _stream()),
               "ufr_marching_cubes_count")
    V, F = int(counts[0]), int(counts[1])
    verts = torch.empty((V, 3), dtype=torch.float32, device=vol.device)
    normals = torch.empty((V, 3), dtype=torch.float32, device=vol.device)
    faces = torch.empty((F, 3), dtype=torch.int32, device=vol.device)
    _lib.check(lib.ufr_marching_cubes_emit(p, dim, float(level), ws.data_ptr(), nbytes, verts.data_ptr() if V else None,
                                           normals.data_ptr() if V else None, faces.data_ptr() if F else None, V, F,
                                           _stream()), "ufr_marching_cubes_emit")
    return verts, faces, normals


def grid_tables(bound_min, bound_max, resolution):
    """The three coordinate tables of a voxel grid as the reference forms them (model.py:893-895): ``torch.linspace`` in
    float32 per axis between the float32 values of the bounds.  ``resolution``: an int or (X, Y, Z).  Host tensors."""
    dim = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
    if len(dim) != 3:
        raise UfrError(f"resolution {resolution!r}: expected an int or three ints")
    lo = torch.as_tensor(bound_min, dtype=torch.float32).reshape(-1)
    hi = torch.as_tensor(bound_max, dtype=torch.float32).reshape(-1)
    if lo.numel() != 3 or hi.numel() != 3:
        raise UfrError("bound_min / bound_max: expected three values each")
    return tuple(torch.linspace(lo[a], hi[a], max(dim[a], 0), dtype=torch.float32).contiguous() for a in range(3))


def similarity_field(frame: FrameHandle, bound_min, bound_max, resolution, min_views: int = 0, return_visibility: bool = False):
    """The similarity field of a frame's matching features on a voxel grid (ufr_similarity_field): ``u`` (X,Y,Z) fp32 on the
    frame's device, z fastest, voxel (i,j,k) at ``grid_tables(...)[0][i], [1][j], [2][k]``; the mean over view pairs and the 8
    channel groups of the gather's pair similarity, without a depth mask, border clamped.  ``min_views > 0``: voxels that
    fewer views see get -1.0.  ``return_visibility``: also ``n_vis`` (X,Y,Z) uint8.  ``u`` starts NaN-filled: a voxel the
    kernel leaves unwritten cannot pass for a value.  Asynchronous on the current stream."""
    gx, gy, gz = grid_tables(bound_min, bound_max, resolution)
    dims = [gx.numel(), gy.numel(), gz.numel()]
    ok = all(d >= 2 for d in dims) and dims[0] * dims[1] * dims[2] < 2 ** 31    # the library refuses these before a launch; so does the allocation here
    u = torch.full(dims if ok else [1], float("nan"), dtype=torch.float32, device=frame.device)
    n_vis = torch.full(dims if ok else [1], 255, dtype=torch.uint8, device=frame.device) if return_visibility else None
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    _lib.check(_lib.load().ufr_similarity_field(C.byref(frame.frame), fp(gx), fp(gy), fp(gz), (C.c_int32 * 3)(*dims), u.data_ptr(),
                                                None if n_vis is None else n_vis.data_ptr(), int(min_views), _stream()),
               "ufr_similarity_field")
    return (u, n_vis) if return_visibility else u


def marching_cubes_table():
    """The kernel's 256-case triangle table as a (256, UFR_MC_TABLE_ROW) int8 array (host only; no GPU needed)."""
    import numpy as np

    lib = _lib.load()
    out = np.empty(256 * MC_TABLE_ROW, np.int8)
    row = lib.ufr_marching_cubes_table(out.ctypes.data_as(C.POINTER(C.c_int8)), out.size)
    if row != MC_TABLE_ROW:
        _lib.check(row if row < 0 else -1, "ufr_marching_cubes_table")
    return out.reshape(256, MC_TABLE_ROW)


MC_TABLE_ROW = 16   # UFR_MC_TABLE_ROW of include/ufr.h


# ---- DTU chamfer evaluation (csrc/chamfer.hip; uforecon_amd/dtu_eval.py strings these together)
def _points64(t: torch.Tensor, name: str) -> int:
    p = _dev(t, name, torch.float64)
    if t.dim() != 2 or t.shape[1] != 3:
        raise UfrError(f"{name}: expected shape (N, 3), got {tuple(t.shape)}")
    if t.shape[0] >= 2 ** 31:
        raise UfrError(f"{name}: {t.shape[0]} points: 2^31 or more")
    return p


def _finite_bounds(t: torch.Tensor, name: str):
    mn, mx = t.min(0).values, t.max(0).values
    if not bool(torch.isfinite(mn).all() and torch.isfinite(mx).all()):
        raise UfrError(f"{name}: contains NaN or infinite coordinates")
    return mn, mx


def cell_keys(points: torch.Tensor, origin, cell: float) -> torch.Tensor:
    """ufr_points_cell_keys: the int64 Morton key of every point's grid cell (floor((p - origin) / cell), 21 bits per axis,
    clamped).  ``points`` (N,3) CUDA float64; ``origin`` three floats."""
    p = _points64(points, "points")
    keys = torch.empty(points.shape[0], dtype=torch.int64, device=points.device)
    if points.shape[0]:
        o = (C.c_double * 3)(*[float(v) for v in origin])
        _lib.check(_lib.load().ufr_points_cell_keys(p, points.shape[0], o, float(cell), keys.data_ptr(), _stream()),
                   "ufr_points_cell_keys")
    return keys


def sample_mesh(verts: torch.Tensor, faces: torch.Tensor, density: float) -> torch.Tensor:
    """The point cloud dtu_eval.py:68-91 makes of a mesh: the vertices, then the points sampled on every triangle at
    ``density`` in (triangle, i, j) order (include/ufr.h, ufr_mesh_sample_*).  ``verts`` (V,3) CUDA float64, ``faces`` (F,3)
    CUDA int32 with every index in 0..V-1.  One host synchronisation (the count sizes the output)."""
    pv = _points64(verts, "verts")
    pf = _dev(faces, "faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise UfrError(f"faces: expected shape (F, 3), got {tuple(faces.shape)}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F == 0 or V == 0:
        if F:
            raise UfrError("sample_mesh: faces without vertices")
        return verts.clone()
    if int(faces.min()) < 0 or int(faces.max()) >= V:
        raise UfrError(f"sample_mesh: face indices span {int(faces.min())}..{int(faces.max())}, the mesh has {V} vertices")
    lib = _lib.load()
    nbytes = lib.ufr_mesh_sample_workspace_bytes(F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
    total = C.c_int64(0)
    _lib.check(lib.ufr_mesh_sample_count(pv, pf, V, F, float(density), ws.data_ptr(), nbytes, C.byref(total), _stream()),
               "ufr_mesh_sample_count")
    M = int(total.value)
    if V + M >= 2 ** 31:
        raise UfrError(f"sample_mesh: {V} vertices + {M} samples: 2^31 points or more")
    out = torch.empty((V + M, 3), dtype=torch.float64, device=verts.device)
    out[:V] = verts
    if M:
        _lib.check(lib.ufr_mesh_sample_emit(pv, pf, V, F, float(density), ws.data_ptr(), nbytes, out[V:].data_ptr(), M, _stream()),
                   "ufr_mesh_sample_emit")
    return out


def thin_points(points: torch.Tensor, radius: float, return_rounds: bool = False):
    """The keep-mask of dtu_eval.py:105-115 (bool, (N,)): in the order of ``points`` ((N,3) CUDA float64, already shuffled), a
    point is kept iff no earlier kept point lies within ``radius`` (inclusive).  Exactly the sequential loop's result, run as
    rounds of a fixpoint (include/ufr.h, ufr_points_thin); synchronises once per round."""
    _points64(points, "points")
    N = int(points.shape[0])
    radius = float(radius)
    if not (radius >= 0.0 and radius < float("inf")):
        raise UfrError(f"thin_points: radius {radius}")
    if N == 0:
        keep = torch.zeros(0, dtype=torch.bool, device=points.device)
        return (keep, 0) if return_rounds else keep
    mn, mx = _finite_bounds(points, "points")
    extent = float((mx - mn).max())
    # cells no smaller than the radius (27 cells then hold every neighbour), and no more of them than the 21-bit keys hold
    cell = max(radius * (1.0 + 1e-9), extent / float(2 ** 21 - 4))
    if cell <= 0.0:
        cell = 1.0
    keys = cell_keys(points, (mn - cell).tolist(), cell)
    keys, perm = torch.sort(keys)
    pts = points[perm].contiguous()
    rank = perm.to(torch.int32)
    state = torch.empty(N, dtype=torch.uint8, device=points.device)
    lib = _lib.load()
    nbytes = lib.ufr_points_thin_workspace_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    rounds = C.c_int32(0)
    _lib.check(lib.ufr_points_thin(pts.data_ptr(), keys.data_ptr(), rank.data_ptr(), N, radius, state.data_ptr(), ws.data_ptr(),
                                   nbytes, C.byref(rounds), _stream()), "ufr_points_thin")
    keep = torch.empty(N, dtype=torch.bool, device=points.device)
    keep[perm] = state == 1
    return (keep, int(rounds.value)) if return_rounds else keep


def nn_distance(query: torch.Tensor, ref: torch.Tensor, max_dist: float, return_sums: bool = False):
    """Distance from every ``query`` point to its nearest ``ref`` point ((N,3) CUDA float64 both): exact fp64 wherever it is
    below ``max_dist``, some value >= ``max_dist`` (inf when nothing is near) elsewhere (include/ufr.h, ufr_points_nn_dist).
    ``return_sums``: also a CUDA float64 pair (sum of the distances < max_dist, their count), summed in a fixed order."""
    _points64(query, "query")
    _points64(ref, "ref")
    nq, nr = int(query.shape[0]), int(ref.shape[0])
    max_dist = float(max_dist)
    if not (0.0 < max_dist < 1e150):
        raise UfrError(f"nn_distance: max_dist {max_dist}")
    if nr == 0:
        raise UfrError("nn_distance: empty reference set")
    sums = torch.zeros(2, dtype=torch.float64, device=query.device)
    if nq == 0:
        dist = torch.zeros(0, dtype=torch.float64, device=query.device)
        return (dist, sums) if return_sums else dist
    mn, mx = _finite_bounds(ref, "ref")
    extent = float((mx - mn).max())
    cell = extent / float(2 ** 20) if extent > 0.0 else 1.0      # the octree is adaptive: the cell only sets its finest level
    origin = (mn - cell).tolist()
    rkeys, rperm = torch.sort(cell_keys(ref, origin, cell))
    rpts = ref[rperm].contiguous()
    qperm = torch.sort(cell_keys(query, origin, cell)).indices        # neighbouring queries share a wave
    qpts = query[qperm].contiguous()
    lib = _lib.load()
    nbytes = lib.ufr_points_nn_dist_workspace_bytes(nq)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
    d = torch.empty(nq, dtype=torch.float64, device=query.device)
    o = (C.c_double * 3)(*origin)
    _lib.check(lib.ufr_points_nn_dist(qpts.data_ptr(), nq, rpts.data_ptr(), rkeys.data_ptr(), nr, o, cell, max_dist, d.data_ptr(),
                                      sums.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ufr_points_nn_dist")
    dist = torch.empty_like(d)
    dist[qperm] = d
    return (dist, sums) if return_sums else dist


# ---- point-cloud filtering (csrc/points_filter.hip; uforecon_amd/pcd_filter.py strings these together)
KNN_MAX_K = 32     # UFR_KNN_MAX_K of include/ufr.h


def knn_points(query: torch.Tensor, ref: torch.Tensor, k: int, max_dist: float = float("inf"), exclude_self: bool = False):
    """The ``k`` nearest ``ref`` points of every ``query`` point ((N,3) CUDA float64 both): ``idx`` (nq,k) int32, indices into
    ``ref``, and ``dist`` (nq,k) float64, ascending by (distance, index), in the order of ``query``; a slot with no point within
    ``max_dist`` (inclusive) holds -1 and inf (include/ufr.h, ufr_points_knn).  ``exclude_self``: ``query`` is ``ref`` and
    point i is left out of its own neighbours."""
    _points64(query, "query")
    _points64(ref, "ref")
    nq, nr = int(query.shape[0]), int(ref.shape[0])
    k, max_dist = int(k), float(max_dist)
    if not 1 <= k <= KNN_MAX_K:
        raise UfrError(f"knn_points: k {k} (must be 1 .. {KNN_MAX_K})")
    if not max_dist > 0.0:
        raise UfrError(f"knn_points: max_dist {max_dist}")
    if exclude_self and query is not ref:
        raise UfrError("knn_points: exclude_self needs query to be ref (the same tensor)")
    if nr == 0:
        raise UfrError("knn_points: empty reference set")
    idx = torch.empty((nq, k), dtype=torch.int32, device=query.device)
    dist = torch.empty((nq, k), dtype=torch.float64, device=query.device)
    if nq == 0:
        return idx, dist
    mn, mx = _finite_bounds(ref, "ref")
    extent = float((mx - mn).max())
    cell = extent / float(2 ** 20) if extent > 0.0 else 1.0      # the octree is adaptive: the cell only sets its finest level
    origin = (mn - cell).tolist()
    rkeys, rperm = torch.sort(cell_keys(ref, origin, cell))
    rpts = ref[rperm].contiguous()
    rindex = rperm.to(torch.int32)
    qperm = rperm if query is ref else torch.sort(cell_keys(query, origin, cell)).indices    # neighbouring queries share a wave
    qpts = rpts if query is ref else query[qperm].contiguous()
    self_index = rindex if exclude_self else None
    i_s = torch.empty_like(idx)
    d_s = torch.empty_like(dist)
    o = (C.c_double * 3)(*origin)
    _lib.check(_lib.load().ufr_points_knn(qpts.data_ptr(), nq, rpts.data_ptr(), rkeys.data_ptr(), rindex.data_ptr(), nr, o, cell,
                                          None if self_index is None else self_index.data_ptr(), k, max_dist, i_s.data_ptr(),
                                          d_s.data_ptr(), _stream()), "ufr_points_knn")
    idx[qperm] = i_s
    dist[qperm] = d_s
    return idx, dist


def point_normals(points: torch.Tensor, idx: torch.Tensor, viewpoints: Optional[torch.Tensor] = None):
    """``normal`` (N,3) float64, ``curvature`` (N,) float64 and ``valid`` (N,) uint8 of every point from its neighbour rows
    ``idx`` ((N,k) CUDA int32 as ``knn_points`` returns them, the point itself included; -1 = empty): the eigenvector of the
    smallest eigenvalue of the neighbours' covariance, turned towards the ``viewpoints`` ((V,3) CUDA float64) or, without
    them, so that its largest component is positive (include/ufr.h, ufr_points_normals)."""
    p = _points64(points, "points")
    pi = _dev(idx, "idx", torch.int32)
    N = int(points.shape[0])
    if idx.dim() != 2 or idx.shape[0] != N or not 1 <= idx.shape[1] <= KNN_MAX_K:
        raise UfrError(f"idx: expected shape ({N}, 1 .. {KNN_MAX_K}), got {tuple(idx.shape)}")
    V, pv = 0, None
    if viewpoints is not None:
        pv = _points64(viewpoints, "viewpoints")
        V = int(viewpoints.shape[0])
        if V and not bool(torch.isfinite(viewpoints).all()):
            raise UfrError("viewpoints: contains NaN or infinite coordinates")
    normal = torch.empty((N, 3), dtype=torch.float64, device=points.device)
    curvature = torch.empty(N, dtype=torch.float64, device=points.device)
    valid = torch.empty(N, dtype=torch.uint8, device=points.device)
    if N:
        _lib.check(_lib.load().ufr_points_normals(p, N, pi, int(idx.shape[1]), pv if V else None, V, normal.data_ptr(),
                                                  curvature.data_ptr(), valid.data_ptr(), _stream()), "ufr_points_normals")
    return normal, curvature, valid


def voxel_downsample(points: torch.Tensor, voxel: float, colors: Optional[torch.Tensor] = None,
                     normals: Optional[torch.Tensor] = None):
    """One point per occupied voxel of the grid with origin ``min_bound - voxel / 2``: the mean position, the rounded mean
    colour ((N,3) CUDA uint8, optional) and the renormalised sum of the normals ((N,3) CUDA float64, optional) of its points,
    summed in ascending index order, voxels in Morton-key order (include/ufr.h, ufr_points_voxel_mean).  Returns ``(points,
    colors or None, normals or None, count)``, count int32.  One host synchronisation (the number of voxels)."""
    _points64(points, "points")
    N = int(points.shape[0])
    voxel = float(voxel)
    if not (voxel > 0.0 and voxel < float("inf")):
        raise UfrError(f"voxel_downsample: voxel {voxel}")
    for t, name, dtype in ((colors, "colors", torch.uint8), (normals, "normals", torch.float64)):
        if t is not None:
            _dev(t, name, dtype)
            if tuple(t.shape) != (N, 3):
                raise UfrError(f"{name}: expected shape ({N}, 3), got {tuple(t.shape)}")
    if N == 0:
        return points.clone(), colors, normals, torch.zeros(0, dtype=torch.int32, device=points.device)
    mn, mx = _finite_bounds(points, "points")
    origin = mn - voxel / 2
    cells = float((torch.floor((mx - origin) / voxel) + 1).max())
    if not cells <= float(2 ** 21 - 4):
        raise UfrError(f"voxel_downsample: voxel {voxel} needs {cells:.0f} cells on an axis (at most 2^21 - 4)")
    keys, perm = torch.sort(cell_keys(points, origin.tolist(), voxel), stable=True)
    pts = points[perm].contiguous()
    col = None if colors is None else colors[perm].contiguous()
    nrm = None if normals is None else normals[perm].contiguous()
    lib = _lib.load()
    nbytes = lib.ufr_points_voxel_mean_workspace_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    out_p = torch.empty((N, 3), dtype=torch.float64, device=points.device)
    out_c = None if col is None else torch.empty((N, 3), dtype=torch.uint8, device=points.device)
    out_n = None if nrm is None else torch.empty((N, 3), dtype=torch.float64, device=points.device)
    count = torch.empty(N, dtype=torch.int32, device=points.device)
    total = C.c_int64(0)
    _lib.check(lib.ufr_points_voxel_mean(pts.data_ptr(), keys.data_ptr(), N, None if col is None else col.data_ptr(),
                                         None if nrm is None else nrm.data_ptr(), out_p.data_ptr(),
                                         None if out_c is None else out_c.data_ptr(), None if out_n is None else out_n.data_ptr(),
                                         count.data_ptr(), N, ws.data_ptr(), nbytes, C.byref(total), _stream()),
               "ufr_points_voxel_mean")
    M = int(total.value)
    return (out_p[:M].contiguous(), None if out_c is None else out_c[:M].contiguous(),
            None if out_n is None else out_n[:M].contiguous(), count[:M].contiguous())


# ---- Poisson surface reconstruction (csrc/poisson.hip; uforecon_amd/poisson_mesh.py strings these together)
POISSON_TILE = (8, 4, 64)        # kPsTileX / Y / Z of csrc/ufr_internal.h: the nodes one block of q = A p owns at a time
POISSON_MAX_PARTIALS = 1024      # UFR_POISSON_MAX_PARTIALS of include/ufr.h


def _poisson_dims(dims, who: str):
    d = tuple(int(v) for v in dims)
    if len(d) != 3:
        raise UfrError(f"{who}: dims {dims!r}: expected three ints")
    return d, (C.c_int32 * 3)(*d)


def _poisson_volume(t: torch.Tensor, name: str, shape) -> int:
    p = _dev(t, name, torch.float64)
    if tuple(t.shape) != tuple(shape):
        raise UfrError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return p


def poisson_grid(points: torch.Tensor, resolution: int = 256, pad: int = 4):
    """The grid of a Poisson reconstruction over ``points`` ((N,3) CUDA float64): ``(origin, h, dims)`` with h = the largest
    extent / ``resolution``, origin = min - pad h and dims = ceil(extent / h) + 1 + 2 pad nodes per axis (include/ufr.h,
    ufr_poisson_grid).  Raises UfrError for resolution < 4, pad < 2, coordinates that are not finite, a cloud without extent
    and a grid of 2^31 nodes or more."""
    _points64(points, "points")
    if int(points.shape[0]) == 0:
        raise UfrError("poisson_grid: empty cloud")
    mn, mx = _finite_bounds(points, "points")
    lo, hi = (C.c_double * 3)(*mn.tolist()), (C.c_double * 3)(*mx.tolist())
    origin, h, dims = (C.c_double * 3)(), C.c_double(0.0), (C.c_int32 * 3)()
    _lib.check(_lib.load().ufr_poisson_grid(lo, hi, int(resolution), int(pad), origin, C.byref(h), dims), "ufr_poisson_grid")
    return tuple(origin), float(h.value), tuple(int(d) for d in dims)


def poisson_splat(points: torch.Tensor, normals: torch.Tensor, origin, h: float, dims):
    """``V`` (3,X,Y,Z) and ``W`` (X,Y,Z) float64: the trilinear splat of ``normals`` and of 1 from ``points`` ((N,3) CUDA
    float64 both) onto the grid, every node's sum taken in ascending sample index (include/ufr.h, ufr_poisson_splat): eight
    (node, row) pairs per sample, one stable sort, and the head of every run sums it left to right."""
    pp, pn = _points64(points, "points"), _points64(normals, "normals")
    N = int(points.shape[0])
    if tuple(normals.shape) != (N, 3):
        raise UfrError(f"normals: expected shape ({N}, 3), got {tuple(normals.shape)}")
    d, cd = _poisson_dims(dims, "poisson_splat")
    o = (C.c_double * 3)(*[float(v) for v in origin])
    lib = _lib.load()
    if not 1 <= N < 2 ** 28:
        raise UfrError(f"poisson_splat: {N} samples (must be 1 .. 2^28 - 1)")
    keys = torch.empty(8 * N, dtype=torch.int64, device=points.device)
    _lib.check(lib.ufr_poisson_splat_keys(pp, N, o, float(h), cd, keys.data_ptr(), _stream()), "ufr_poisson_splat_keys")
    keys, rows = torch.sort(keys, stable=True)
    V = torch.empty((3,) + d, dtype=torch.float64, device=points.device)
    W = torch.empty(d, dtype=torch.float64, device=points.device)
    _lib.check(lib.ufr_poisson_splat(pp, pn, N, o, float(h), cd, keys.data_ptr(), rows.data_ptr(), V.data_ptr(), W.data_ptr(),
                                     _stream()), "ufr_poisson_splat")
    return V, W


def poisson_divergence(V: torch.Tensor, h: float) -> torch.Tensor:
    """``b`` (X,Y,Z) = div ``V`` ((3,X,Y,Z) CUDA float64) by central differences over 2 h, V = 0 outside the grid."""
    if not isinstance(V, torch.Tensor) or V.dim() != 4 or V.shape[0] != 3:
        raise UfrError("V: expected a (3, X, Y, Z) tensor")
    d, cd = _poisson_dims(V.shape[1:], "poisson_divergence")
    b = torch.empty(d, dtype=torch.float64, device=V.device)
    _lib.check(_lib.load().ufr_poisson_divergence(_dev(V, "V", torch.float64), cd, float(h), b.data_ptr(), _stream()),
               "ufr_poisson_divergence")
    return b


def poisson_laplacian(p: torch.Tensor, h: float) -> torch.Tensor:
    """One application of the solver's matrix: ``A p`` for ``p`` (X,Y,Z) CUDA float64, A = the negated 7-point Laplacian over
    h^2 with zeros outside the grid (include/ufr.h, ufr_poisson_laplacian)."""
    if not isinstance(p, torch.Tensor) or p.dim() != 3:
        raise UfrError("p: expected an (X, Y, Z) tensor")
    d, cd = _poisson_dims(p.shape, "poisson_laplacian")
    q = torch.empty(d, dtype=torch.float64, device=p.device)
    _lib.check(_lib.load().ufr_poisson_laplacian(_dev(p, "p", torch.float64), cd, float(h), q.data_ptr(), _stream()),
               "ufr_poisson_laplacian")
    return q


def poisson_workspace_bytes(dims) -> int:
    """Bytes of the solver's workspace for a grid of ``dims`` nodes (0: the library refuses the grid)."""
    return int(_lib.load().ufr_poisson_workspace_bytes(_poisson_dims(dims, "poisson_workspace_bytes")[1]))


def poisson_solve(b: torch.Tensor, h: float, tol: float = 1e-6, max_iter: Optional[int] = None, check_every: int = 16,
                  workspace: Optional[torch.Tensor] = None):
    """``(x, info)``: the solution of A x = -b by conjugate gradients from 0 (include/ufr.h, ufr_poisson_solve), ``b`` (X,Y,Z)
    CUDA float64; ``info`` = dict(iterations, residual = |r| / |b| of the recurrence, converged).  The host looks at the
    residual every ``check_every`` iterations; ``max_iter`` defaults to 8 max(dims) and reaching it is reported, not raised.
    ``workspace``: a CUDA uint8 tensor of at least ``poisson_workspace_bytes(dims)`` bytes (allocated when None)."""
    if not isinstance(b, torch.Tensor) or b.dim() != 3:
        raise UfrError("b: expected an (X, Y, Z) tensor")
    d, cd = _poisson_dims(b.shape, "poisson_solve")
    pb = _dev(b, "b", torch.float64)
    lib = _lib.load()
    nbytes = lib.ufr_poisson_workspace_bytes(cd)
    if nbytes == 0:
        raise UfrError(f"poisson_solve: grid {d} unsupported (every dim >= 2, fewer than 2^31 nodes)")
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=b.device)
    pw = _dev(workspace, "workspace", torch.uint8)
    if max_iter is None:
        max_iter = 8 * max(d)
    x = torch.empty(d, dtype=torch.float64, device=b.device)
    it, res, conv = C.c_int32(0), C.c_double(0.0), C.c_int32(0)
    _lib.check(lib.ufr_poisson_solve(pb, cd, float(h), float(tol), int(max_iter), int(check_every), x.data_ptr(), pw,
                                     workspace.numel(), C.byref(it), C.byref(res), C.byref(conv), _stream()), "ufr_poisson_solve")
    return x, dict(iterations=int(it.value), residual=float(res.value), converged=bool(conv.value))


def poisson_sample(vol: torch.Tensor, origin, h: float, points: torch.Tensor, return_mean: bool = False):
    """The trilinear value of ``vol`` ((X,Y,Z) CUDA float64, node (i,j,k) at origin + h (i,j,k)) at every point ((N,3) CUDA
    float64), positions clamped to the grid (include/ufr.h, ufr_poisson_sample).  ``return_mean``: also their mean, a CUDA
    float64 scalar summed in a fixed order."""
    if not isinstance(vol, torch.Tensor) or vol.dim() != 3:
        raise UfrError("vol: expected an (X, Y, Z) tensor")
    d, cd = _poisson_dims(vol.shape, "poisson_sample")
    pv, pp = _dev(vol, "vol", torch.float64), _points64(points, "points")
    N = int(points.shape[0])
    values = torch.empty(N, dtype=torch.float64, device=vol.device)
    mean = torch.zeros((), dtype=torch.float64, device=vol.device)
    if N:
        lib = _lib.load()
        nbytes = lib.ufr_poisson_sample_workspace_bytes(N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
        o = (C.c_double * 3)(*[float(v) for v in origin])
        _lib.check(lib.ufr_poisson_sample(pv, cd, o, float(h), pp, N, values.data_ptr(), mean.data_ptr() if return_mean else None,
                                          ws.data_ptr(), nbytes, _stream()), "ufr_poisson_sample")
    return (values, mean) if return_mean else values


# ---- depth-map fusion (csrc/depth_fusion.hip; uforecon_amd/depth_fusion.py strings these together)
DEPTH_MAX_SOURCES = 64     # UFR_DEPTH_MAX_SOURCES of include/ufr.h
DEPTH_PAIR_DOUBLES = 68    # UFR_DEPTH_PAIR_DOUBLES


def depth_consistency(ref_depth: torch.Tensor, src_depths, mats: torch.Tensor, geo_pixel_thres: float = 1,
                      geo_depth_thres: float = 0.01, geo_mask_thres: int = 2, return_pair_masks: bool = False):
    """ufr_depth_consistency: one reference view against its S source views.  ``ref_depth`` (H,W) and every entry of
    ``src_depths`` (its own (Hs,Ws)): CUDA float32, contiguous; ``mats`` (S, 68) CUDA float64, the six host-made matrices
    of every pair (include/ufr.h).  Returns ``mask_sum`` int32, ``mask`` uint8 and ``depth_avg`` float64, all (H,W), and with
    ``return_pair_masks`` the (S,H,W) uint8 per-pair masks.  Does not synchronise."""
    p_ref = _dev(ref_depth, "ref_depth")
    if ref_depth.dim() != 2:
        raise UfrError(f"ref_depth: expected shape (H, W), got {tuple(ref_depth.shape)}")
    src_depths = list(src_depths)
    S = len(src_depths)
    if not 1 <= S <= DEPTH_MAX_SOURCES:
        raise UfrError(f"depth_consistency: {S} source views (must be 1 .. {DEPTH_MAX_SOURCES})")
    ptrs = (C.c_void_p * S)()
    hw = (C.c_int32 * (2 * S))()
    for k, t in enumerate(src_depths):
        ptrs[k] = _dev(t, f"src_depths[{k}]")
        if t.dim() != 2:
            raise UfrError(f"src_depths[{k}]: expected shape (H, W), got {tuple(t.shape)}")
        hw[2 * k], hw[2 * k + 1] = int(t.shape[0]), int(t.shape[1])
    p_mats = _dev(mats, "mats", torch.float64)
    if tuple(mats.shape) != (S, DEPTH_PAIR_DOUBLES):
        raise UfrError(f"mats: expected shape ({S}, {DEPTH_PAIR_DOUBLES}), got {tuple(mats.shape)}")
    H, W = int(ref_depth.shape[0]), int(ref_depth.shape[1])
    dev = ref_depth.device
    mask_sum = torch.empty((H, W), dtype=torch.int32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    depth_avg = torch.empty((H, W), dtype=torch.float64, device=dev)
    pair = torch.empty((S, H, W), dtype=torch.uint8, device=dev) if return_pair_masks else None
    _lib.check(_lib.load().ufr_depth_consistency(p_ref, H, W, ptrs, hw, p_mats, S, float(geo_pixel_thres), float(geo_depth_thres),
                                                 int(geo_mask_thres), mask_sum.data_ptr(), mask.data_ptr(), depth_avg.data_ptr(),
                                                 None if pair is None else pair.data_ptr(), _stream()), "ufr_depth_consistency")
    return (mask_sum, mask, depth_avg, pair) if return_pair_masks else (mask_sum, mask, depth_avg)


def depth_points(mask: torch.Tensor, depth_avg: torch.Tensor, color: torch.Tensor, inv_k, inv_e):
    """ufr_depth_points_*: the pixels with ``mask`` != 0 as points, in row-major pixel order.  ``mask`` (H,W) CUDA uint8,
    ``depth_avg`` (H,W) CUDA float64, ``color`` (H,W,3) CUDA uint8; ``inv_k`` 3x3 and ``inv_e`` 4x4: host arrays (widened to
    float64).  Returns ``xyz`` (N,3) float32 and ``rgb`` (N,3) uint8 on the device; N = 0 gives empty tensors.  Synchronises
    (the count sizes the outputs)."""
    import numpy as np

    p_mask = _dev(mask, "mask", torch.uint8)
    p_avg = _dev(depth_avg, "depth_avg", torch.float64)
    p_col = _dev(color, "color", torch.uint8)
    if mask.dim() != 2 or depth_avg.shape != mask.shape or tuple(color.shape) != (*mask.shape, 3):
        raise UfrError(f"depth_points: mask {tuple(mask.shape)}, depth_avg {tuple(depth_avg.shape)}, color {tuple(color.shape)}: "
                       "expected (H, W), (H, W), (H, W, 3)")
    ik = np.ascontiguousarray(np.asarray(inv_k, np.float64))
    ie = np.ascontiguousarray(np.asarray(inv_e, np.float64))
    if ik.shape != (3, 3) or ie.shape != (4, 4):
        raise UfrError(f"depth_points: inv_k {ik.shape}, inv_e {ie.shape}: expected (3, 3) and (4, 4)")
    H, W = int(mask.shape[0]), int(mask.shape[1])
    lib = _lib.load()
    nbytes = lib.ufr_depth_points_workspace_bytes(H, W)
    if nbytes == 0:
        raise UfrError(f"depth_points: image {H}x{W} unsupported (H, W >= 1, fewer than 2^31 pixels)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    n = C.c_int64(0)
    _lib.check(lib.ufr_depth_points_count(p_mask, H, W, ws.data_ptr(), nbytes, C.byref(n), _stream()), "ufr_depth_points_count")
    N = int(n.value)
    xyz = torch.empty((N, 3), dtype=torch.float32, device=mask.device)
    rgb = torch.empty((N, 3), dtype=torch.uint8, device=mask.device)
    dp = C.POINTER(C.c_double)
    _lib.check(lib.ufr_depth_points_emit(p_mask, p_avg, p_col, H, W, ik.ctypes.data_as(dp), ie.ctypes.data_as(dp), ws.data_ptr(),
                                         nbytes, xyz.data_ptr() if N else None, rgb.data_ptr() if N else None, N, _stream()),
               "ufr_depth_points_emit")
    return xyz, rgb


# ---- DTU mesh cleaning (csrc/mesh_clean.hip; uforecon_amd/clean_mesh.py strings these together)
MASK_MAX_KERNEL = 127      # UFR_MASK_MAX_KERNEL of include/ufr.h
MESH_MAX_VIEWS = 64        # UFR_MESH_MAX_VIEWS


def _faces(faces: torch.Tensor, V: int, who: str, rows: bool = False) -> int:
    """F of an (F,3) int32 face array, on any device; raises on a wrong dtype or shape, on a face index outside 0..V-1 (one
    host synchronisation) and, with ``rows`` (the caller hands the 3F corner slots to the library), on 3F >= 2^31"""
    _typed(faces, "faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise UfrError(f"faces: expected shape (F, 3), got {tuple(faces.shape)}")
    F = int(faces.shape[0])
    if rows and 3 * F >= 2 ** 31:
        raise UfrError(f"{who}: {F} faces: (2^31 - 1) / 3 or more")
    if F and (V == 0 or int(faces.min()) < 0 or int(faces.max()) >= V):
        raise UfrError(f"{who}: face indices span {int(faces.min())}..{int(faces.max())}, the mesh has {V} vertices")
    return F


def _mesh(verts: torch.Tensor, faces: torch.Tensor, who: str, rows: bool = False):
    """pointers and sizes of a mesh on the GPU, checked by ``_points64`` and ``_faces``"""
    pv = _points64(verts, "verts")
    pf = _dev(faces, "faces", torch.int32)
    V = int(verts.shape[0])
    return pv, pf, V, _faces(faces, V, who, rows)


def _corner_runs(faces: torch.Tensor, V: int):
    """The one order every per-vertex mesh stage walks: the 3F corner slots 3f + e sorted stably by the vertex they name,
    ``slots`` (3F,) int64, and where each vertex's run starts, ``runs`` (V+1,) int64; both contiguous, on the device of
    ``faces`` (any device).  A kernel that walks a run in ascending slot sums in one order, whatever the scheduling."""
    svert, slots = torch.sort(faces.reshape(-1).to(torch.int64), stable=True)
    runs = torch.searchsorted(svert, torch.arange(V + 1, dtype=torch.int64, device=faces.device))
    return slots.contiguous(), runs.contiguous()


def _ring_setup(verts: torch.Tensor, faces: torch.Tensor, pinned: Optional[torch.Tensor], who: str):
    """What the stages that move vertices over their ring share: the checks of the mesh and of ``pinned``, a zeroed
    ``border`` (V,) uint8 and ``pos_a``, a copy of ``verts`` -- the first of the two buffers the steps ping-pong.  Returns V, F,
    border, pos_a and whether the mesh is empty (the input's positions are then the answer)."""
    _, _, V, F = _mesh(verts, faces, who, rows=True)
    if pinned is not None:
        _dev(pinned, "pinned", torch.uint8)
        if tuple(pinned.shape) != (V,):
            raise UfrError(f"pinned: expected shape ({V},), got {tuple(pinned.shape)}")
    border = torch.zeros(V, dtype=torch.uint8, device=verts.device)
    return V, F, border, verts.clone(), V == 0 or F == 0


def _ring_result(pos_a: torch.Tensor, pos_b: torch.Tensor, n_steps: int) -> torch.Tensor:
    """the buffer that holds the positions after ``n_steps`` steps that began in ``pos_a``"""
    return pos_a if n_steps % 2 == 0 else pos_b


def mask_half_widths(k: int):
    """ufr_mask_half_widths: the rows of cv.getStructuringElement(MORPH_ELLIPSE, (k, k)) as half-widths (a list of k ints)."""
    k = int(k)
    if not (1 <= k <= MASK_MAX_KERNEL and k % 2 == 1):
        raise UfrError(f"mask_half_widths: k {k} (must be odd, 1 .. {MASK_MAX_KERNEL})")
    out = (C.c_int32 * k)()
    _lib.check(_lib.load().ufr_mask_half_widths(k, out), "ufr_mask_half_widths")
    return list(out)


def dilate_mask(image: torch.Tensor, k: int = 11, threshold: int = 128, return_dilated: bool = False):
    """ufr_mask_dilate: cv.dilate of ``image`` ((H,W) CUDA uint8) with the k x k MORPH_ELLIPSE element, pixels outside the image
    ignored, then ``> threshold``.  Returns the (H,W) uint8 0/1 mask, with ``return_dilated`` also the dilated uint8 image.
    Does not synchronise."""
    p = _dev(image, "image", torch.uint8)
    if image.dim() != 2 or image.shape[0] < 1 or image.shape[1] < 1:
        raise UfrError(f"image: expected shape (H, W) with H, W >= 1, got {tuple(image.shape)}")
    k = int(k)
    if not (1 <= k <= MASK_MAX_KERNEL and k % 2 == 1):
        raise UfrError(f"dilate_mask: k {k} (must be odd, 1 .. {MASK_MAX_KERNEL})")
    H, W = int(image.shape[0]), int(image.shape[1])
    mask = torch.empty((H, W), dtype=torch.uint8, device=image.device)
    dil = torch.empty((H, W), dtype=torch.uint8, device=image.device) if return_dilated else None
    _lib.check(_lib.load().ufr_mask_dilate(p, H, W, k, int(threshold), None if dil is None else dil.data_ptr(), mask.data_ptr(),
                                           _stream()), "ufr_mask_dilate")
    return (mask, dil) if return_dilated else mask


def mesh_vertex_votes(verts: torch.Tensor, P: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
    """ufr_mesh_vertex_votes: in how many views a vertex projects into the mask or onto the reference's ones border
    (include/ufr.h).  ``verts`` (V,3) CUDA float64, ``P`` (NV,3,4) or (NV,4,4) CUDA float32 (the first three rows are used),
    ``masks`` (NV,H,W) CUDA uint8.  Returns (V,) int32.  Does not synchronise."""
    pv = _points64(verts, "verts")
    if not isinstance(P, torch.Tensor) or P.dim() != 3 or tuple(P.shape[1:]) not in ((3, 4), (4, 4)):
        raise UfrError(f"P: expected shape (NV, 3, 4) or (NV, 4, 4), got {tuple(getattr(P, 'shape', ()))}")
    if P.shape[1] == 4:
        P = P[:, :3].contiguous()
    pp = _dev(P, "P")
    pm = _dev(masks, "masks", torch.uint8)
    NV = int(P.shape[0])
    if masks.dim() != 3 or masks.shape[0] != NV or masks.shape[1] < 1 or masks.shape[2] < 1:
        raise UfrError(f"masks: expected shape ({NV}, H, W), got {tuple(masks.shape)}")
    if not 1 <= NV <= MESH_MAX_VIEWS:
        raise UfrError(f"mesh_vertex_votes: {NV} views (must be 1 .. {MESH_MAX_VIEWS})")
    V = int(verts.shape[0])
    votes = torch.zeros(V, dtype=torch.int32, device=verts.device)
    if V:
        _lib.check(_lib.load().ufr_mesh_vertex_votes(pv, V, pp, pm, NV, int(masks.shape[1]), int(masks.shape[2]), votes.data_ptr(),
                                                     _stream()), "ufr_mesh_vertex_votes")
    return votes


def mesh_first_hit(verts: torch.Tensor, faces: torch.Tensor, k_inv, c2w, mask: torch.Tensor,
                   face_hit: Optional[torch.Tensor] = None):
    """ufr_mesh_first_hit: the face that the ray of every pixel with ``mask`` != 0 hits first, for one view.  ``verts`` (V,3)
    CUDA float64, ``faces`` (F,3) CUDA int32, ``mask`` (H,W) CUDA uint8; ``k_inv`` 3x3 and ``c2w`` 4x4: host arrays, narrowed to
    float32 (what gen_rays_from_single_image is given).  Returns ``face_id`` (H,W) int32 (-1: no ray or no hit) and ``face_hit``
    (F,) uint8, in which every hit face is set to 1; pass the previous view's ``face_hit`` to accumulate.  A face index out
    of range raises.  One host synchronisation (the index check)."""
    import numpy as np

    pv, pf, V, F = _mesh(verts, faces, "mesh_first_hit")
    pm = _dev(mask, "mask", torch.uint8)
    if mask.dim() != 2 or mask.shape[0] < 1 or mask.shape[1] < 1:
        raise UfrError(f"mask: expected shape (H, W) with H, W >= 1, got {tuple(mask.shape)}")
    ki = np.ascontiguousarray(np.asarray(k_inv, np.float32))
    cw = np.ascontiguousarray(np.asarray(c2w, np.float32))
    if ki.shape != (3, 3) or cw.shape != (4, 4):
        raise UfrError(f"mesh_first_hit: k_inv {ki.shape}, c2w {cw.shape}: expected (3, 3) and (4, 4)")
    H, W = int(mask.shape[0]), int(mask.shape[1])
    dev = verts.device
    if face_hit is None:
        face_hit = torch.zeros(F, dtype=torch.uint8, device=dev)
    ph = _dev(face_hit, "face_hit", torch.uint8)
    if tuple(face_hit.shape) != (F,):
        raise UfrError(f"face_hit: expected shape ({F},), got {tuple(face_hit.shape)}")
    face_id = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    if F == 0:
        return face_id, face_hit
    lib = _lib.load()
    nbytes = lib.ufr_mesh_first_hit_workspace_bytes(F, H, W)
    if nbytes == 0:
        raise UfrError(f"mesh_first_hit: F {F}, image {H}x{W} unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fp = C.POINTER(C.c_float)
    _lib.check(lib.ufr_mesh_first_hit(pv, pf, V, F, ki.ctypes.data_as(fp), cw.ctypes.data_as(fp), pm, H, W, face_id.data_ptr(), ph,
                                      ws.data_ptr(), nbytes, _stream()), "ufr_mesh_first_hit")
    return face_id, face_hit


def mesh_face_components(verts: torch.Tensor, faces: torch.Tensor, return_rounds: bool = False):
    """Connected components of the faces over trimesh's face adjacency (include/ufr.h, ufr_mesh_edge_keys and
    ufr_mesh_face_components): vertices with exactly equal coordinates are one vertex (``torch.unique``), two faces are adjacent
    iff they share an undirected edge that exactly two faces have.  ``verts`` (V,3) CUDA float64, ``faces`` (F,3) CUDA int32.
    Returns ``labels`` (F,) int32: the lowest face index of the component, -1 for a face without adjacency (a face with two
    equal vertices has none).  A face index out of range raises.  Synchronises once per union-find round."""
    pv, pf, V, F = _mesh(verts, faces, "mesh_face_components")
    dev = verts.device
    if F == 0:
        labels = torch.zeros(0, dtype=torch.int32, device=dev)
        return (labels, 0) if return_rounds else labels
    vid = torch.unique(verts, dim=0, return_inverse=True)[1].to(torch.int32).contiguous()
    lib = _lib.load()
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    _lib.check(lib.ufr_mesh_edge_keys(pf, vid.data_ptr(), V, F, keys.data_ptr(), _stream()), "ufr_mesh_edge_keys")
    skeys, order = torch.sort(keys)
    nbytes = lib.ufr_mesh_face_components_workspace_bytes(F)
    if nbytes == 0:
        raise UfrError(f"mesh_face_components: {F} faces unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    rounds = C.c_int32(0)
    _lib.check(lib.ufr_mesh_face_components(skeys.data_ptr(), order.data_ptr(), F, labels.data_ptr(), ws.data_ptr(), nbytes,
                                            C.byref(rounds), _stream()), "ufr_mesh_face_components")
    return (labels, int(rounds.value)) if return_rounds else labels


# ---- mesh rendering (csrc/raster.hip; uforecon_amd/render_trajectory.py strings these together)
def raster_vertex_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """ufr_raster_vertex_normals: area-weighted vertex normals, (V,3) float64 -- the normalised sum of (b - a) x (c - a) over the
    faces that use the vertex, (0,0,0) for a vertex without faces or with a zero sum.  ``verts`` (V,3) CUDA float64, ``faces``
    (F,3) CUDA int32.  The corner slots are sorted by vertex here (stable), so the sums do not depend on scheduling.  A face
    index out of range raises.  One host synchronisation (the index check)."""
    pv, pf, V, F = _mesh(verts, faces, "raster_vertex_normals", rows=True)
    normals = torch.zeros((V, 3), dtype=torch.float64, device=verts.device)
    if V == 0 or F == 0:
        return normals
    slots, runs = _corner_runs(faces, V)
    _lib.check(_lib.load().ufr_raster_vertex_normals(pv, pf, V, F, slots.data_ptr(), runs.data_ptr(), normals.data_ptr(),
                                                     _stream()), "ufr_raster_vertex_normals")
    return normals


def raster_frames(verts: torch.Tensor, faces: torch.Tensor, k_inv, c2ws, H: int, W: int, normals: Optional[torch.Tensor] = None,
                  colors: Optional[torch.Tensor] = None, base_color=(1.0, 1.0, 1.0), background=(255, 255, 255),
                  ambient: float = 0.25, return_depth: bool = False, return_face_ids: bool = False,
                  return_normals: bool = False, check_indices: bool = True):
    """ufr_raster_frames: ``n`` shaded views of a mesh in one call (include/ufr.h states every rule).  ``verts`` (V,3) CUDA
    float64, ``faces`` (F,3) CUDA int32; ``k_inv`` 3x3 and ``c2ws`` (n,4,4): host arrays, narrowed to float32, with the meaning
    ``mesh_first_hit`` gives them; ``normals`` (V,3) CUDA float64 or None (flat shading); ``colors`` (V,3) CUDA uint8 or None
    (``base_color``).  Returns a dict: ``image`` (n,H,W,3) uint8, and when asked ``depth`` (n,H,W) float32 z-depth (0: no hit),
    ``face_id`` (n,H,W) int32 (-1: no hit), ``normal`` (n,H,W,3) float32 in camera coordinates, facing the camera.  One index
    check (a host synchronisation) per call, none with ``check_indices=False`` (a caller that has checked the mesh already);
    the frames themselves synchronise nowhere."""
    import numpy as np

    if check_indices:
        pv, pf, V, F = _mesh(verts, faces, "raster_frames")
    else:
        pv, pf, V, F = _points64(verts, "verts"), _dev(faces, "faces", torch.int32), int(verts.shape[0]), int(faces.shape[0])
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise UfrError(f"faces: expected shape (F, 3), got {tuple(faces.shape)}")
    ki = np.ascontiguousarray(np.asarray(k_inv, np.float32))
    cw = np.ascontiguousarray(np.asarray(c2ws, np.float32))
    if ki.shape != (3, 3) or cw.ndim != 3 or cw.shape[1:] != (4, 4) or cw.shape[0] < 1:
        raise UfrError(f"raster_frames: k_inv {ki.shape}, c2ws {cw.shape}: expected (3, 3) and (n, 4, 4) with n >= 1")
    n, H, W = int(cw.shape[0]), int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise UfrError(f"raster_frames: image {H}x{W} (H, W >= 1, H * W < 2^31)")
    if not 0.0 <= float(ambient) <= 1.0:
        raise UfrError(f"raster_frames: ambient {ambient} (must be 0 .. 1)")
    base = np.ascontiguousarray(np.asarray(base_color, np.float32).reshape(-1))
    bg = np.ascontiguousarray(np.asarray(background).reshape(-1))
    if base.shape != (3,) or not ((base >= 0) & (base <= 1)).all():
        raise UfrError(f"raster_frames: base_color {base_color!r} (three values in 0 .. 1)")
    if bg.shape != (3,) or not ((bg >= 0) & (bg <= 255) & (bg == np.rint(bg))).all():
        raise UfrError(f"raster_frames: background {background!r} (three integers in 0 .. 255)")
    bg = np.ascontiguousarray(bg.astype(np.uint8))
    pn = pc = None
    if normals is not None:
        pn = _points64(normals, "normals")
        if normals.shape[0] != V:
            raise UfrError(f"normals: expected shape ({V}, 3), got {tuple(normals.shape)}")
    if colors is not None:
        pc = _dev(colors, "colors", torch.uint8)
        if tuple(colors.shape) != (V, 3):
            raise UfrError(f"colors: expected shape ({V}, 3), got {tuple(colors.shape)}")
    dev = verts.device
    bgt = torch.from_numpy(bg).to(dev)
    out = {"image": bgt.expand(n, H, W, 3).contiguous()}
    if return_depth:
        out["depth"] = torch.zeros((n, H, W), dtype=torch.float32, device=dev)
    if return_face_ids:
        out["face_id"] = torch.full((n, H, W), -1, dtype=torch.int32, device=dev)
    if return_normals:
        out["normal"] = torch.zeros((n, H, W, 3), dtype=torch.float32, device=dev)
    if F == 0 or V == 0:
        return out
    lib = _lib.load()
    nbytes = lib.ufr_raster_frames_workspace_bytes(F, H, W)
    if nbytes == 0:
        raise UfrError(f"raster_frames: F {F}, image {H}x{W} unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fp, ptr = C.POINTER(C.c_float), lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    _lib.check(lib.ufr_raster_frames(pv, pf, V, F, pn, pc, ki.ctypes.data_as(fp), cw.ctypes.data_as(fp), n, H, W, base.ctypes.data_as(fp),
                                     bg.ctypes.data_as(C.POINTER(C.c_uint8)), float(ambient), out["image"].data_ptr(), ptr("depth"),
                                     ptr("face_id"), ptr("normal"), ws.data_ptr(), nbytes, _stream()), "ufr_raster_frames")
    return out


def raster_downsample(images: torch.Tensor, s: int) -> torch.Tensor:
    """ufr_raster_downsample: (n,s*H,s*W,3) CUDA uint8 -> (n,H,W,3) uint8, the mean of every s x s block in integer arithmetic,
    round half to even; ``s`` in 1..4 (1 copies).  Does not synchronise."""
    p = _dev(images, "images", torch.uint8)
    s = int(s)
    if not 1 <= s <= 4:
        raise UfrError(f"raster_downsample: s {s} (must be 1 .. 4)")
    if images.dim() != 4 or images.shape[3] != 3 or images.shape[0] < 1 or images.shape[1] < s or images.shape[2] < s \
            or images.shape[1] % s or images.shape[2] % s:
        raise UfrError(f"images: expected shape (n, {s}*H, {s}*W, 3) with n, H, W >= 1, got {tuple(images.shape)}")
    n, H, W = int(images.shape[0]), int(images.shape[1]) // s, int(images.shape[2]) // s
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=images.device)
    _lib.check(_lib.load().ufr_raster_downsample(p, n, H, W, s, out.data_ptr(), _stream()), "ufr_raster_downsample")
    return out


# ---- point-cloud rendering (csrc/splat.hip; uforecon_amd/render_trajectory.py's render_points is the caller)
def splat_frames(points: torch.Tensor, k, w2cs, H: int, W: int, colors: Optional[torch.Tensor] = None, radius: int = 1,
                 z_min: float = 0.0, base_color=(1.0, 1.0, 1.0), background=(255, 255, 255), edl_strength: float = 0.0,
                 edl_radius: int = 1, return_depth: bool = False, return_point_ids: bool = False):
    """ufr_splat_frames: ``n`` z-buffered splat views of a point cloud in one call (include/ufr.h states every rule).
    ``points`` (N,3) CUDA float64; ``k`` 3x3 and ``w2cs`` (n,4,4): host float64 arrays, ``k`` already divided by ``k[2,2]``,
    ``w2cs`` the world-to-camera matrices; ``colors`` (N,3) CUDA uint8 or None (``base_color``, 0..1); ``radius`` 0..4 the
    footprint; ``edl_strength`` >= 0 and ``edl_radius`` >= 1 the eye-dome lighting.  Returns a dict: ``image`` (n,H,W,3) uint8,
    and when asked ``depth`` (n,H,W) float32 z-depth (0: empty), ``point_id`` (n,H,W) int32 (-1: empty).  No points: the
    background, without a library call.  Synchronises nowhere."""
    import numpy as np

    pp = _points64(points, "points")
    N = int(points.shape[0])
    kk = np.ascontiguousarray(np.asarray(k, np.float64))
    wc = np.ascontiguousarray(np.asarray(w2cs, np.float64))
    if kk.shape != (3, 3) or wc.ndim != 3 or wc.shape[1:] != (4, 4) or wc.shape[0] < 1:
        raise UfrError(f"splat_frames: k {kk.shape}, w2cs {wc.shape}: expected (3, 3) and (n, 4, 4) with n >= 1")
    n, H, W = int(wc.shape[0]), int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise UfrError(f"splat_frames: image {H}x{W} (H, W >= 1, H * W < 2^31)")
    base = np.ascontiguousarray(np.asarray(base_color, np.float32).reshape(-1))
    bg = np.ascontiguousarray(np.asarray(background).reshape(-1))
    if base.shape != (3,) or not ((base >= 0) & (base <= 1)).all():
        raise UfrError(f"splat_frames: base_color {base_color!r} (three values in 0 .. 1)")
    if bg.shape != (3,) or not ((bg >= 0) & (bg <= 255) & (bg == np.rint(bg))).all():
        raise UfrError(f"splat_frames: background {background!r} (three integers in 0 .. 255)")
    bg = np.ascontiguousarray(bg.astype(np.uint8))
    pc = None
    if colors is not None:
        pc = _dev(colors, "colors", torch.uint8)
        if tuple(colors.shape) != (N, 3):
            raise UfrError(f"colors: expected shape ({N}, 3), got {tuple(colors.shape)}")
    dev = points.device
    out = {"image": torch.from_numpy(bg).to(dev).expand(n, H, W, 3).contiguous()}
    if return_depth:
        out["depth"] = torch.zeros((n, H, W), dtype=torch.float32, device=dev)
    if return_point_ids:
        out["point_id"] = torch.full((n, H, W), -1, dtype=torch.int32, device=dev)
    if N == 0:
        return out
    lib = _lib.load()
    nbytes = lib.ufr_splat_frames_workspace_bytes(H, W)
    if nbytes == 0:
        raise UfrError(f"splat_frames: image {H}x{W} unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dp, ptr = C.POINTER(C.c_double), lambda key: out[key].data_ptr() if key in out else None  # noqa: E731
    _lib.check(lib.ufr_splat_frames(pp, N, pc, kk.ctypes.data_as(dp), wc.ctypes.data_as(dp), n, H, W, int(radius), float(z_min),
                                    base.ctypes.data_as(C.POINTER(C.c_float)), bg.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    float(edl_strength), int(edl_radius), out["image"].data_ptr(), ptr("depth"), ptr("point_id"),
                                    ws.data_ptr(), nbytes, _stream()), "ufr_splat_frames")
    return out


# ---- mesh colouring (csrc/mesh_color.hip; uforecon_amd/color_mesh.py strings these together)
MESH_COLOR_BLOCK = 256           # kColorThreads of csrc/ufr_internal.h: the vertices one block owns
MESH_COLOR_MAX_POWER = 8         # UFR_MESH_COLOR_MAX_POWER of include/ufr.h
MESH_COLOR_MODES = {"mean": 0, "best": 1}   # UFR_MESH_COLOR_MEAN / _BEST


def mesh_vertex_colors(verts: torch.Tensor, normals: Optional[torch.Tensor], images: torch.Tensor, depth: Optional[torch.Tensor],
                       k, w2c, centre, z_min: float = 0.0, depth_tol: float = 0.005, min_cos: float = 0.2, power: int = 2,
                       mode: str = "mean", fill=(128, 128, 128)):
    """ufr_color_vertices: per-vertex colour from ``n`` photographs (include/ufr.h states every rule).  ``verts`` (V,3) CUDA
    float64; ``normals`` (V,3) CUDA float64 or None (every view weighs 1); ``images`` (n,H,W,3) CUDA uint8; ``depth`` (n,H,W)
    CUDA float32 z-depth of the mesh from the same cameras (``raster_frames(return_depth=True)``; 0: no hit) or None (no
    occlusion test); ``k`` (n,3,3), ``w2c`` (n,4,4), ``centre`` (n,3): host float64 arrays, ``k`` already divided by
    ``k[2,2]``.  ``mode`` "mean" (weights cos^power) or "best" (the view of largest weight).  Returns ``colors`` (V,3) uint8
    and ``views_used`` (V,) uint8; a vertex no view saw gets ``fill``.  Synchronises nowhere."""
    import numpy as np

    pv = _points64(verts, "verts")
    V = int(verts.shape[0])
    pn = pd = None
    if normals is not None:
        pn = _points64(normals, "normals")
        if normals.shape[0] != V:
            raise UfrError(f"normals: expected shape ({V}, 3), got {tuple(normals.shape)}")
    pi = _dev(images, "images", torch.uint8)
    if images.dim() != 4 or images.shape[3] != 3:
        raise UfrError(f"images: expected shape (n, H, W, 3), got {tuple(images.shape)}")
    n, H, W = (int(s) for s in images.shape[:3])
    if not 1 <= n <= MESH_MAX_VIEWS:
        raise UfrError(f"mesh_vertex_colors: {n} views (must be 1 .. {MESH_MAX_VIEWS})")
    if H < 2 or W < 2 or H * W >= 2 ** 31:
        raise UfrError(f"mesh_vertex_colors: image {H}x{W} (H, W >= 2, H * W < 2^31)")
    if depth is not None:
        pd = _dev(depth, "depth", torch.float32)
        if tuple(depth.shape) != (n, H, W):
            raise UfrError(f"depth: expected shape ({n}, {H}, {W}), got {tuple(depth.shape)}")
    kk = np.ascontiguousarray(np.asarray(k, np.float64))
    wc = np.ascontiguousarray(np.asarray(w2c, np.float64))
    cc = np.ascontiguousarray(np.asarray(centre, np.float64))
    if kk.shape != (n, 3, 3) or wc.shape != (n, 4, 4) or cc.shape != (n, 3):
        raise UfrError(f"mesh_vertex_colors: k {kk.shape}, w2c {wc.shape}, centre {cc.shape}: expected ({n}, 3, 3), ({n}, 4, 4) "
                       f"and ({n}, 3)")
    if not (float(z_min) >= 0.0 and float(z_min) < float("inf")):
        raise UfrError(f"mesh_vertex_colors: z_min {z_min} (must be >= 0 and finite)")
    if not (float(depth_tol) >= 0.0 and float(depth_tol) < float("inf")):
        raise UfrError(f"mesh_vertex_colors: depth_tol {depth_tol} (must be >= 0 and finite)")
    if not 0.0 <= float(min_cos) <= 1.0:
        raise UfrError(f"mesh_vertex_colors: min_cos {min_cos} (must be 0 .. 1)")
    if int(power) != power or not 0 <= int(power) <= MESH_COLOR_MAX_POWER:
        raise UfrError(f"mesh_vertex_colors: power {power} (an integer in 0 .. {MESH_COLOR_MAX_POWER})")
    if mode not in MESH_COLOR_MODES:
        raise UfrError(f"mesh_vertex_colors: mode {mode!r} (one of {sorted(MESH_COLOR_MODES)})")
    fl = np.ascontiguousarray(np.asarray(fill).reshape(-1))
    if fl.shape != (3,) or not ((fl >= 0) & (fl <= 255) & (fl == np.rint(fl))).all():
        raise UfrError(f"mesh_vertex_colors: fill {fill!r} (three integers in 0 .. 255)")
    fl = np.ascontiguousarray(fl.astype(np.uint8))
    dev = verts.device
    colors = torch.empty((V, 3), dtype=torch.uint8, device=dev)
    used = torch.empty(V, dtype=torch.uint8, device=dev)
    if V == 0:
        return colors, used
    lib = _lib.load()
    nbytes = lib.ufr_color_vertices_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dp = C.POINTER(C.c_double)
    _lib.check(lib.ufr_color_vertices(pv, pn, V, pi, pd, kk.ctypes.data_as(dp), wc.ctypes.data_as(dp), cc.ctypes.data_as(dp), n, H,
                                          W, float(z_min), float(depth_tol), float(min_cos), int(power), MESH_COLOR_MODES[mode],
                                          fl.ctypes.data_as(C.POINTER(C.c_uint8)), colors.data_ptr(), used.data_ptr(), ws.data_ptr(),
                                          nbytes, _stream()), "ufr_color_vertices")
    return colors, used


def mesh_color_fill(faces: torch.Tensor, colors: torch.Tensor, views_used: torch.Tensor, rounds: int):
    """Up to ``rounds`` rounds of ufr_color_fill_round: a vertex without colour (``views_used`` == 0) takes the mean of
    its coloured neighbours, a neighbour once per face that shares the edge, rounded half to even; one round reaches one
    edge further.  ``faces`` (F,3) CUDA int32, ``colors`` (V,3) CUDA uint8, ``views_used`` (V,) CUDA uint8.  Returns
    ``colors`` (V,3) uint8, ``state`` (V,) uint8 (0: still empty) and the rounds run -- a round that fills nothing is the
    last, and is counted.  The corner slots are sorted by vertex here, once (stable).  A face index out of range raises.
    One host read per round, and one for the index check."""
    pf = _dev(faces, "faces", torch.int32)
    _dev(colors, "colors", torch.uint8)
    _dev(views_used, "views_used", torch.uint8)
    V = int(views_used.shape[0])
    if tuple(colors.shape) != (V, 3) or views_used.dim() != 1:
        raise UfrError(f"mesh_color_fill: colors {tuple(colors.shape)}, views_used {tuple(views_used.shape)}: expected (V, 3) and (V,)")
    rounds = int(rounds)
    if rounds < 0:
        raise UfrError(f"mesh_color_fill: rounds {rounds} (must be >= 0)")
    F = _faces(faces, V, "mesh_color_fill", rows=True)
    cur, state = colors.clone(), (views_used != 0).to(torch.uint8)
    if rounds == 0 or V == 0 or F == 0:
        return cur, state, 0
    slots, runs = _corner_runs(faces, V)
    nxt, nstate = torch.empty_like(cur), torch.empty_like(state)
    filled = torch.zeros(1, dtype=torch.int32, device=colors.device)
    lib, run = _lib.load(), 0
    while run < rounds:
        filled.zero_()
        _lib.check(lib.ufr_color_fill_round(pf, V, F, slots.data_ptr(), runs.data_ptr(), cur.data_ptr(), state.data_ptr(),
                                                 nxt.data_ptr(), nstate.data_ptr(), filled.data_ptr(), _stream()),
                   "ufr_color_fill_round")
        cur, nxt, state, nstate = nxt, cur, nstate, state
        run += 1
        if int(filled.item()) == 0:
            break
    return cur, state, run


# ---- mesh simplification (csrc/mesh_simplify.hip; uforecon_amd/simplify_mesh.py is the caller)
SIMPLIFY_BLOCK = 256             # kSimplifyThreads of csrc/ufr_internal.h: the items one block of a scanning kernel owns
SIMPLIFY_PLACEMENTS = {"quadric": 0, "mean": 1}   # UFR_SIMPLIFY_QUADRIC / _MEAN
SIMPLIFY_MAX_CELLS = 2 ** 21 - 4                  # cells on an axis, as voxel_downsample refuses them
SIMPLIFY_BISECTION_STEPS = 32


def _simplify_ws(n: int, device):
    nbytes = _lib.load().ufr_simplify_workspace_bytes(int(n))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _origin3(origin):
    return (C.c_double * 3)(*[float(v) for v in origin])


def simplify_clusters(sorted_keys: torch.Tensor, order: torch.Tensor):
    """ufr_simplify_clusters: ``sorted_keys`` and ``order`` (V,) CUDA int64 as a stable sort of the cell keys returns them.
    Returns ``cluster`` (V,) int32, the cluster of every input vertex, and ``cluster_key`` (C,) int64.  One synchronisation."""
    pk, po = _dev(sorted_keys, "sorted_keys", torch.int64), _dev(order, "order", torch.int64)
    V = int(sorted_keys.shape[0])
    if sorted_keys.dim() != 1 or tuple(order.shape) != (V,) or not 1 <= V < 2 ** 31:
        raise UfrError(f"simplify_clusters: sorted_keys {tuple(sorted_keys.shape)}, order {tuple(order.shape)}: expected (V,) twice, "
                       f"V in 1 .. 2^31 - 1")
    dev = sorted_keys.device
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    ckey = torch.empty(V, dtype=torch.int64, device=dev)
    ws, nbytes = _simplify_ws(V, dev)
    total = C.c_int64(0)
    _lib.check(_lib.load().ufr_simplify_clusters(pk, po, V, cluster.data_ptr(), ckey.data_ptr(), V, ws.data_ptr(), nbytes,
                                                 C.byref(total), _stream()), "ufr_simplify_clusters")
    return cluster, ckey[:int(total.value)].contiguous()


def simplify_face_keys(faces: torch.Tensor, cluster: torch.Tensor) -> torch.Tensor:
    """ufr_simplify_face_keys: (3F,) int64, up to three ``cluster << 32 | face`` rows per face, 2^63 - 1 in the unused slots."""
    pf, pc = _dev(faces, "faces", torch.int32), _dev(cluster, "cluster", torch.int32)
    V, F = int(cluster.shape[0]), int(faces.shape[0])
    keys = torch.empty(3 * F, dtype=torch.int64, device=faces.device)
    _lib.check(_lib.load().ufr_simplify_face_keys(pf, pc, V, F, keys.data_ptr(), _stream()), "ufr_simplify_face_keys")
    return keys


def simplify_quadrics(verts: torch.Tensor, faces: torch.Tensor, cluster_key: torch.Tensor, origin, cell: float,
                      sorted_keys: torch.Tensor):
    """ufr_simplify_quadrics: ``quadrics`` (C,10) float64 and ``n_faces`` (C,) int32, every cluster's ten sums taken over its
    faces in ascending face index; ``sorted_keys`` (3F,) = the sorted rows of ``simplify_face_keys``."""
    pv, pf = _points64(verts, "verts"), _dev(faces, "faces", torch.int32)
    pk, ps = _dev(cluster_key, "cluster_key", torch.int64), _dev(sorted_keys, "sorted_keys", torch.int64)
    V, F, Cn = int(verts.shape[0]), int(faces.shape[0]), int(cluster_key.shape[0])
    if tuple(sorted_keys.shape) != (3 * F,):
        raise UfrError(f"sorted_keys: expected shape ({3 * F},), got {tuple(sorted_keys.shape)}")
    q = torch.empty((Cn, 10), dtype=torch.float64, device=verts.device)
    nf = torch.empty(Cn, dtype=torch.int32, device=verts.device)
    _lib.check(_lib.load().ufr_simplify_quadrics(pv, pf, pk, V, F, Cn, _origin3(origin), float(cell), ps, q.data_ptr(), nf.data_ptr(),
                                                 _stream()), "ufr_simplify_quadrics")
    return q, nf


def simplify_place(quadrics: torch.Tensor, n_faces: torch.Tensor, mean: torch.Tensor, cluster_key: torch.Tensor, origin, cell: float,
                   placement: str = "quadric"):
    """ufr_simplify_place: ``position`` (C,3) float64 and ``placed`` (C,) uint8 (1: the regularised quadric's minimiser was
    taken, 0: the mean)."""
    if placement not in SIMPLIFY_PLACEMENTS:
        raise UfrError(f"simplify_place: placement {placement!r} (one of {sorted(SIMPLIFY_PLACEMENTS)})")
    pq, pn = _dev(quadrics, "quadrics", torch.float64), _dev(n_faces, "n_faces", torch.int32)
    pm, pk = _points64(mean, "mean"), _dev(cluster_key, "cluster_key", torch.int64)
    Cn = int(mean.shape[0])
    if tuple(quadrics.shape) != (Cn, 10) or tuple(n_faces.shape) != (Cn,) or tuple(cluster_key.shape) != (Cn,):
        raise UfrError(f"simplify_place: quadrics {tuple(quadrics.shape)}, n_faces {tuple(n_faces.shape)}, cluster_key "
                       f"{tuple(cluster_key.shape)}: expected ({Cn}, 10), ({Cn},) and ({Cn},)")
    pos = torch.empty((Cn, 3), dtype=torch.float64, device=mean.device)
    placed = torch.empty(Cn, dtype=torch.uint8, device=mean.device)
    _lib.check(_lib.load().ufr_simplify_place(pq, pn, pm, pk, Cn, _origin3(origin), float(cell), SIMPLIFY_PLACEMENTS[placement],
                                              pos.data_ptr(), placed.data_ptr(), _stream()), "ufr_simplify_place")
    return pos, placed


def simplify_face_triples(faces: torch.Tensor, cluster: torch.Tensor):
    """ufr_simplify_face_triples: ``triples`` (F,3) int32 in cluster numbers, smallest first ((-1,-1,-1): collapsed), and the
    two sort keys ``key_a``, ``key_bc`` (F,) int64 (2^63 - 1: collapsed)."""
    pf, pc = _dev(faces, "faces", torch.int32), _dev(cluster, "cluster", torch.int32)
    V, F = int(cluster.shape[0]), int(faces.shape[0])
    dev = faces.device
    tri = torch.empty((F, 3), dtype=torch.int32, device=dev)
    ka, kbc = torch.empty(F, dtype=torch.int64, device=dev), torch.empty(F, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().ufr_simplify_face_triples(pf, pc, V, F, tri.data_ptr(), ka.data_ptr(), kbc.data_ptr(), _stream()),
               "ufr_simplify_face_triples")
    return tri, ka, kbc


def simplify_face_heads(key_a: torch.Tensor, key_bc: torch.Tensor) -> torch.Tensor:
    """The two stable sorts (by ``key_bc``, then by ``key_a``) and ufr_simplify_face_heads: ``keep`` (F,) uint8 by input index,
    1 for the lowest input index of every distinct rotated triple."""
    pa, pb = _dev(key_a, "key_a", torch.int64), _dev(key_bc, "key_bc", torch.int64)
    F = int(key_a.shape[0])
    if tuple(key_bc.shape) != (F,):
        raise UfrError(f"key_bc: expected shape ({F},), got {tuple(key_bc.shape)}")
    o1 = torch.sort(key_bc, stable=True).indices
    o2 = torch.sort(key_a[o1], stable=True).indices
    order = o1[o2].contiguous()
    keep = torch.empty(F, dtype=torch.uint8, device=key_a.device)
    _lib.check(_lib.load().ufr_simplify_face_heads(pa, pb, order.data_ptr(), F, keep.data_ptr(), _stream()), "ufr_simplify_face_heads")
    return keep


def simplify_compact_faces(triples: torch.Tensor, keep: torch.Tensor, n_clusters: int):
    """ufr_simplify_compact_faces: the kept triples in ascending input index: ``faces`` (F',3) int32 in cluster numbers,
    ``face_map`` (F',) int32, ``referenced`` (C,) uint8.  One synchronisation."""
    pt, pk = _dev(triples, "triples", torch.int32), _dev(keep, "keep", torch.uint8)
    F, Cn = int(keep.shape[0]), int(n_clusters)
    if tuple(triples.shape) != (F, 3):
        raise UfrError(f"triples: expected shape ({F}, 3), got {tuple(triples.shape)}")
    dev = triples.device
    out = torch.empty((F, 3), dtype=torch.int32, device=dev)
    fmap = torch.empty(F, dtype=torch.int32, device=dev)
    ref = torch.empty(Cn, dtype=torch.uint8, device=dev)
    ws, nbytes = _simplify_ws(F, dev)
    total = C.c_int64(0)
    _lib.check(_lib.load().ufr_simplify_compact_faces(pt, pk, F, Cn, out.data_ptr(), fmap.data_ptr(), F, ref.data_ptr(), ws.data_ptr(),
                                                      nbytes, C.byref(total), _stream()), "ufr_simplify_compact_faces")
    n = int(total.value)
    return out[:n].contiguous(), fmap[:n].contiguous(), ref


def simplify_compact_vertices(referenced: torch.Tensor, position: torch.Tensor, colors: Optional[torch.Tensor], placed: torch.Tensor,
                              count: torch.Tensor, cluster: torch.Tensor, faces: torch.Tensor):
    """ufr_simplify_compact_vertices: the referenced clusters renumbered in key order.  ``faces`` (F',3) int32 in cluster
    numbers is rewritten IN PLACE to output vertices.  Returns ``verts`` (V',3), ``colors`` or None, ``placed``, ``count`` and
    ``vertex_map`` (V,) int32.  One synchronisation."""
    pr, pp = _dev(referenced, "referenced", torch.uint8), _points64(position, "position")
    pc = None if colors is None else _dev(colors, "colors", torch.uint8)
    ppl, pcn = _dev(placed, "placed", torch.uint8), _dev(count, "count", torch.int32)
    pcl, pf = _dev(cluster, "cluster", torch.int32), _dev(faces, "faces", torch.int32)
    Cn, V, Fp = int(referenced.shape[0]), int(cluster.shape[0]), int(faces.shape[0])
    if tuple(position.shape) != (Cn, 3) or tuple(placed.shape) != (Cn,) or tuple(count.shape) != (Cn,) or (
            colors is not None and tuple(colors.shape) != (Cn, 3)) or faces.dim() != 2 or faces.shape[1] != 3:
        raise UfrError(f"simplify_compact_vertices: shapes do not agree with {Cn} clusters")
    dev = position.device
    ov = torch.empty((Cn, 3), dtype=torch.float64, device=dev)
    oc = None if colors is None else torch.empty((Cn, 3), dtype=torch.uint8, device=dev)
    op = torch.empty(Cn, dtype=torch.uint8, device=dev)
    on = torch.empty(Cn, dtype=torch.int32, device=dev)
    cv = torch.empty(Cn, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    ws, nbytes = _simplify_ws(Cn, dev)
    total = C.c_int64(0)
    _lib.check(_lib.load().ufr_simplify_compact_vertices(pr, Cn, pp, pc, ppl, pcn, pcl, V, pf if Fp else None, Fp, ov.data_ptr(),
                                                         None if oc is None else oc.data_ptr(), op.data_ptr(), on.data_ptr(), Cn,
                                                         cv.data_ptr(), vmap.data_ptr(), ws.data_ptr(), nbytes, C.byref(total),
                                                         _stream()), "ufr_simplify_compact_vertices")
    n = int(total.value)
    return ov[:n].contiguous(), None if oc is None else oc[:n].contiguous(), op[:n].contiguous(), on[:n].contiguous(), vmap


def _simplify_mesh_args(verts, faces, colors, who: str):
    _points64(verts, "verts")
    _dev(faces, "faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise UfrError(f"faces: expected shape (F, 3), got {tuple(faces.shape)}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F >= 2 ** 31:
        raise UfrError(f"{who}: {F} faces: 2^31 or more")
    if colors is not None:
        _dev(colors, "colors", torch.uint8)
        if tuple(colors.shape) != (V, 3):
            raise UfrError(f"colors: expected shape ({V}, 3), got {tuple(colors.shape)}")
    mn = mx = None
    if V:
        mn, mx = _finite_bounds(verts, "verts")
    if F and (V == 0 or int(faces.min()) < 0 or int(faces.max()) >= V):
        raise UfrError(f"{who}: face indices span {int(faces.min())}..{int(faces.max())}, the mesh has {V} vertices")
    return V, F, mn, mx


def _simplify_sorted_keys(verts, mn, mx, cell: float, who: str):
    origin = mn - cell / 2
    cells = float((torch.floor((mx - origin) / cell) + 1).max())
    if not cells <= float(SIMPLIFY_MAX_CELLS):
        raise UfrError(f"{who}: cell {cell} needs {cells:.0f} cells on an axis (at most 2^21 - 4)")
    origin = origin.tolist()
    keys, order = torch.sort(cell_keys(verts, origin, cell), stable=True)
    return origin, keys, order


def simplify_count_cells(verts: torch.Tensor, cell: float, bounds=None) -> int:
    """The number of occupied cells of the clustering grid at ``cell``: the keys, one sort, and the run-head count of
    ufr_points_voxel_mean (capacity 0: nothing is summed).  One synchronisation."""
    _points64(verts, "verts")
    mn, mx = bounds if bounds is not None else _finite_bounds(verts, "verts")
    _, keys, _ = _simplify_sorted_keys(verts, mn, mx, float(cell), "simplify_count_cells")
    V = int(verts.shape[0])
    lib = _lib.load()
    nbytes = lib.ufr_points_voxel_mean_workspace_bytes(V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
    total = C.c_int64(0)
    _lib.check(lib.ufr_points_voxel_mean(verts.data_ptr(), keys.data_ptr(), V, None, None, None, None, None, None, 0, ws.data_ptr(),
                                         nbytes, C.byref(total), _stream()), "ufr_points_voxel_mean")
    return int(total.value)


def simplify_target_cell(verts: torch.Tensor, target_vertices: int, bounds=None) -> float:
    """The cell edge at which the clustering grid has at most ``target_vertices`` occupied cells: a geometric bisection of
    exactly 32 steps between ``max_extent * 2^-20`` and ``2 * diagonal`` (one cell holds everything there), ``mid = sqrt(lo *
    hi)``, ``hi = mid`` when the count at ``mid`` is <= the target, else ``lo = mid``; the result is ``hi``."""
    import math

    N = int(target_vertices)
    if N < 1:
        raise UfrError(f"simplify_target_cell: target_vertices {target_vertices} (must be >= 1)")
    _points64(verts, "verts")
    if int(verts.shape[0]) == 0:
        raise UfrError("simplify_target_cell: no vertices")
    mn, mx = bounds if bounds is not None else _finite_bounds(verts, "verts")
    e = (mx - mn).tolist()
    lo, hi = max(e) * 2.0 ** -20, 2.0 * math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    if not (lo > 0.0 and hi < float("inf")):
        raise UfrError(f"simplify_target_cell: the vertices span {e}: no extent to divide")
    for _ in range(SIMPLIFY_BISECTION_STEPS):
        mid = math.sqrt(lo * hi)
        if simplify_count_cells(verts, mid, (mn, mx)) <= N:
            hi = mid
        else:
            lo = mid
    return hi


def mesh_simplify(verts: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None, cell: Optional[float] = None,
                  target_vertices: Optional[int] = None, placement: str = "quadric"):
    """Vertex clustering with quadric placement (include/ufr.h, "mesh simplification", states every rule).  ``verts`` (V,3)
    CUDA float64, ``faces`` (F,3) CUDA int32, ``colors`` (V,3) CUDA uint8 or None; exactly one of ``cell`` (> 0) and
    ``target_vertices``; ``placement`` "quadric" or "mean".  Returns a dict: ``verts`` (V',3) float64, ``faces`` (F',3) int32,
    ``colors`` (V',3) uint8 or None, ``vertex_map`` (V,) int32 (the output vertex of every input vertex or -1), ``face_map``
    (F',) int32 (the input index of every output face), ``placed`` (V',) uint8 (1: the quadric's minimiser, 0: the mean),
    ``count`` (V',) int32 (input vertices per output vertex), ``cell`` (0.0: ``target_vertices`` >= V, the mesh came back
    unchanged), and the counts ``clusters``, ``collapsed_faces``, ``duplicate_faces``.  A vertex that is not finite, a face index
    outside 0 .. V-1, a cell that is not positive and finite, wrong dtypes or shapes raise UfrError before any kernel of the
    library runs."""
    if placement not in SIMPLIFY_PLACEMENTS:
        raise UfrError(f"mesh_simplify: placement {placement!r} (one of {sorted(SIMPLIFY_PLACEMENTS)})")
    if (cell is None) == (target_vertices is None):
        raise UfrError("mesh_simplify: give exactly one of cell and target_vertices")
    if cell is not None and not (float(cell) > 0.0 and float(cell) < float("inf")):
        raise UfrError(f"mesh_simplify: cell {cell} (must be positive and finite)")
    if target_vertices is not None and (int(target_vertices) != target_vertices or int(target_vertices) < 1):
        raise UfrError(f"mesh_simplify: target_vertices {target_vertices} (an integer >= 1)")
    V, F, mn, mx = _simplify_mesh_args(verts, faces, colors, "mesh_simplify")
    dev = verts.device
    i32 = dict(dtype=torch.int32, device=dev)
    if target_vertices is not None and V <= int(target_vertices):
        return dict(verts=verts.clone(), faces=faces.clone(), colors=None if colors is None else colors.clone(),
                    vertex_map=torch.arange(V, **i32), face_map=torch.arange(F, **i32),
                    placed=torch.zeros(V, dtype=torch.uint8, device=dev), count=torch.ones(V, **i32), cell=0.0, clusters=V,
                    collapsed_faces=0, duplicate_faces=0)
    cell = float(cell) if cell is not None else simplify_target_cell(verts, int(target_vertices), (mn, mx))
    empty = dict(verts=verts.new_zeros((0, 3)), faces=torch.zeros((0, 3), **i32),
                 colors=None if colors is None else colors.new_zeros((0, 3)), vertex_map=torch.full((V,), -1, **i32),
                 face_map=torch.zeros(0, **i32), placed=torch.zeros(0, dtype=torch.uint8, device=dev), count=torch.zeros(0, **i32),
                 cell=cell, clusters=0, collapsed_faces=F, duplicate_faces=0)
    if V == 0 or F == 0:
        return empty
    origin, keys, order = _simplify_sorted_keys(verts, mn, mx, cell, "mesh_simplify")
    cluster, ckey = simplify_clusters(keys, order)
    Cn = int(ckey.shape[0])
    # the count, the mean and the rounded mean colour of every cluster: the voxel mean of the sorted vertices
    lib = _lib.load()
    pts = verts[order].contiguous()
    col = None if colors is None else colors[order].contiguous()
    mean = torch.empty((Cn, 3), dtype=torch.float64, device=dev)
    ccol = None if col is None else torch.empty((Cn, 3), dtype=torch.uint8, device=dev)
    count = torch.empty(Cn, **i32)
    nbytes = lib.ufr_points_voxel_mean_workspace_bytes(V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    total = C.c_int64(0)
    _lib.check(lib.ufr_points_voxel_mean(pts.data_ptr(), keys.data_ptr(), V, None if col is None else col.data_ptr(), None,
                                         mean.data_ptr(), None if ccol is None else ccol.data_ptr(), None, count.data_ptr(), Cn,
                                         ws.data_ptr(), nbytes, C.byref(total), _stream()), "ufr_points_voxel_mean")
    if int(total.value) != Cn:
        raise UfrError(f"mesh_simplify: {int(total.value)} voxel means for {Cn} clusters")
    fkeys = torch.sort(simplify_face_keys(faces, cluster), stable=True).values
    quadrics, n_faces = simplify_quadrics(verts, faces, ckey, origin, cell, fkeys)
    position, placed = simplify_place(quadrics, n_faces, mean, ckey, origin, cell, placement)
    triples, key_a, key_bc = simplify_face_triples(faces, cluster)
    keep = simplify_face_heads(key_a, key_bc)
    out_faces, face_map, referenced = simplify_compact_faces(triples, keep, Cn)
    out_verts, out_colors, out_placed, out_count, vertex_map = simplify_compact_vertices(referenced, position, ccol, placed, count,
                                                                                         cluster, out_faces)
    collapsed = int((key_a == 2 ** 63 - 1).sum())
    return dict(verts=out_verts, faces=out_faces, colors=out_colors, vertex_map=vertex_map, face_map=face_map, placed=out_placed,
                count=out_count, cell=cell, clusters=Cn, collapsed_faces=collapsed,
                duplicate_faces=F - collapsed - int(out_faces.shape[0]))


# ---- mesh smoothing (csrc/mesh_smooth.hip; uforecon_amd/smooth_mesh.py is the caller)
MESH_ROW_BLOCK = 256                                # kMeshRowThreads of csrc/mesh_rows.h: the rows, faces or vertices one block owns
MESH_ROW_CHUNK = 1024                               # kMeshRowChunk: the rows a block of a staged walk holds in LDS at a time
SMOOTH_BLOCK, SMOOTH_CHUNK = MESH_ROW_BLOCK, MESH_ROW_CHUNK
SMOOTH_WEIGHTS = {"uniform": 0, "cotangent": 1}     # UFR_SMOOTH_UNIFORM / _COTANGENT
SMOOTH_METHODS = ("taubin", "laplacian")
SMOOTH_BOUNDARIES = ("fixed", "free")
SMOOTH_PASS_BAND = 0.1                              # Taubin's k_pb: the default mu is 1 / (k_pb - 1 / lam)


def smooth_factors(method: str = "taubin", iterations: int = 10, lam: float = 0.5, mu: Optional[float] = None):
    """The step factors of a smoothing call, a list of floats: ``iterations`` times ``lam`` ("laplacian") or ``lam, mu``
    ("taubin"; ``mu`` None: ``1 / (0.1 - 1 / lam)``).  Raises UfrError with one line unless ``0 < lam <= 1``, ``mu < -lam``
    and ``iterations`` is an integer >= 0."""
    if method not in SMOOTH_METHODS:
        raise UfrError(f"mesh_smooth: method {method!r} (one of {sorted(SMOOTH_METHODS)})")
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 0:
        raise UfrError(f"mesh_smooth: iterations {iterations} (an integer >= 0)")
    lam = float(lam)
    if not 0.0 < lam <= 1.0:
        raise UfrError(f"mesh_smooth: lam {lam} (must be in (0, 1])")
    if method == "laplacian":
        return [lam] * int(iterations)
    mu = 1.0 / (SMOOTH_PASS_BAND - 1.0 / lam) if mu is None else float(mu)
    if not (mu < -lam and mu > float("-inf")):
        raise UfrError(f"mesh_smooth: mu {mu} (must be finite and below -lam = {-lam})")
    return [lam, mu] * int(iterations)


def mesh_smooth(verts: torch.Tensor, faces: torch.Tensor, method: str = "taubin", weights: str = "cotangent", iterations: int = 10,
                lam: float = 0.5, mu: Optional[float] = None, boundary: str = "fixed", pinned: Optional[torch.Tensor] = None):
    """Laplacian or Taubin smoothing of the vertex positions (include/ufr.h, "mesh smoothing", states every rule).  ``verts``
    (V,3) CUDA float64, ``faces`` (F,3) CUDA int32; ``method`` "taubin" (every iteration one step with ``lam``, then one with
    ``mu``) or "laplacian" (``iterations`` steps with ``lam``); ``weights`` "cotangent" (from the input positions, clamped to 0
    .. 64) or "uniform"; ``boundary`` "fixed" (border vertices stay) or "free"; ``pinned`` (V,) CUDA uint8 or None: further
    vertices that stay.  Returns a dict: ``verts`` (V,3) float64 (a new tensor; the input's bits when nothing moves) and
    ``border`` (V,) uint8.  The corner slots are sorted by vertex here, once (stable); all steps go out in one library call.
    A face index outside 0 .. V-1, ``lam`` outside (0, 1], ``mu`` >= -``lam``, a negative ``iterations``, wrong dtypes or
    shapes raise UfrError before any kernel of the library runs.  One host synchronisation (the index check)."""
    if weights not in SMOOTH_WEIGHTS:
        raise UfrError(f"mesh_smooth: weights {weights!r} (one of {sorted(SMOOTH_WEIGHTS)})")
    if boundary not in SMOOTH_BOUNDARIES:
        raise UfrError(f"mesh_smooth: boundary {boundary!r} (one of {sorted(SMOOTH_BOUNDARIES)})")
    factors = smooth_factors(method, iterations, lam, mu)
    V, F, border, pos_a, empty = _ring_setup(verts, faces, pinned, "mesh_smooth")
    if empty:
        return dict(verts=pos_a, border=border)
    mode = SMOOTH_WEIGHTS[weights]
    slots, runs = _corner_runs(faces, V)
    lib = _lib.load()
    nbytes = lib.ufr_smooth_workspace_bytes(V, F, mode)
    if nbytes == 0:
        raise UfrError(f"mesh_smooth: V {V}, F {F} unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
    _lib.check(lib.ufr_smooth_rows(verts.data_ptr(), faces.data_ptr(), V, F, slots.data_ptr(), runs.data_ptr(), mode,
                                        border.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ufr_smooth_rows")
    n = len(factors)
    if n == 0:
        return dict(verts=pos_a, border=border)
    pos_b = torch.empty_like(pos_a)
    _lib.check(lib.ufr_smooth_steps(V, F, runs.data_ptr(), mode, border.data_ptr() if boundary == "fixed" else None,
                                         None if pinned is None else pinned.data_ptr(), (C.c_double * n)(*factors), n,
                                         pos_a.data_ptr(), pos_b.data_ptr(), ws.data_ptr(), nbytes, _stream()),
               "ufr_smooth_steps")
    return dict(verts=_ring_result(pos_a, pos_b, n), border=border)


# ---- mesh denoising (csrc/mesh_denoise.hip; uforecon_amd/denoise_mesh.py is the caller)
DENOISE_BLOCK, DENOISE_CHUNK = MESH_ROW_BLOCK, MESH_ROW_CHUNK
DENOISE_SIGMA_R = 0.35                              # the chord of about 20 degrees: a neighbour turned that far weighs e^-1/2


def _denoise_count(name: str, n) -> int:
    if isinstance(n, bool) or int(n) != n or int(n) < 0 or int(n) >= 2 ** 31:
        raise UfrError(f"mesh_denoise: {name} {n} (an integer >= 0)")
    return int(n)


def _denoise_sigma(name: str, s) -> float:
    if s is None:
        raise UfrError(f"mesh_denoise: {name} is required")
    s = float(s)
    two = 2.0 * (s * s)
    if not (s > 0.0 and 0.0 < two < float("inf")):
        raise UfrError(f"mesh_denoise: {name} {s} (must be finite and above 0)")
    return two


def mesh_denoise(verts: torch.Tensor, faces: torch.Tensor, normal_iterations: int = 5, vertex_iterations: int = 10,
                 sigma_s: Optional[float] = None, sigma_r: float = DENOISE_SIGMA_R, boundary: str = "fixed",
                 pinned: Optional[torch.Tensor] = None):
    """Feature-preserving denoising of the vertex positions: ``normal_iterations`` steps of the bilateral normal filter, then
    ``vertex_iterations`` steps that move the vertices to the filtered normals (include/ufr.h, "mesh denoising", states every
    rule).  ``verts`` (V,3) CUDA float64, ``faces`` (F,3) CUDA int32; ``sigma_s`` (required here; ``denoise_mesh`` defaults it to
    the mean edge length) scales the distance between centroids and ``sigma_r`` the difference of unit normals; ``boundary``
    "fixed" (border vertices stay) or "free"; ``pinned`` (V,) CUDA uint8 or None: further vertices that stay.  Returns a
    dict: ``verts`` (V,3) float64 (a new tensor; the input's bits when ``vertex_iterations`` is 0), ``normals`` (F,3) float64
    (the filtered face normals, zeros for a dead face) and ``border`` (V,) uint8.  Empty ``faces`` or ``verts`` give the input
    positions back.  The corner slots are sorted by vertex here, once (stable); each phase goes out in one library call.  A
    face index outside 0 .. V-1, a sigma that is not finite or not above 0, a negative iteration count, wrong dtypes or shapes
    raise UfrError before any kernel of the library runs.  One host synchronisation (the index check)."""
    if boundary not in SMOOTH_BOUNDARIES:
        raise UfrError(f"mesh_denoise: boundary {boundary!r} (one of {sorted(SMOOTH_BOUNDARIES)})")
    n_normal = _denoise_count("normal_iterations", normal_iterations)
    n_vertex = _denoise_count("vertex_iterations", vertex_iterations)
    two_ss, two_rr = _denoise_sigma("sigma_s", sigma_s), _denoise_sigma("sigma_r", sigma_r)
    V, F, border, pos_a, empty = _ring_setup(verts, faces, pinned, "mesh_denoise")
    normals = torch.zeros((F, 3), dtype=torch.float64, device=verts.device)
    if empty:
        return dict(verts=pos_a, normals=normals, border=border)
    slots, runs = _corner_runs(faces, V)
    lib = _lib.load()
    nbytes = lib.ufr_denoise_workspace_bytes(V, F)
    if nbytes == 0:
        raise UfrError(f"mesh_denoise: V {V}, F {F} unsupported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
    _lib.check(lib.ufr_denoise_faces(verts.data_ptr(), faces.data_ptr(), V, F, slots.data_ptr(), runs.data_ptr(), normals.data_ptr(),
                                     border.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ufr_denoise_faces")
    if n_normal:
        _lib.check(lib.ufr_denoise_normals(faces.data_ptr(), V, F, runs.data_ptr(), two_ss, two_rr, n_normal, normals.data_ptr(),
                                           ws.data_ptr(), nbytes, _stream()), "ufr_denoise_normals")
    if n_vertex == 0:
        return dict(verts=pos_a, normals=normals, border=border)
    pos_b = torch.empty_like(pos_a)
    _lib.check(lib.ufr_denoise_vertices(V, F, runs.data_ptr(), normals.data_ptr(), border.data_ptr() if boundary == "fixed" else None,
                                        None if pinned is None else pinned.data_ptr(), n_vertex, pos_a.data_ptr(), pos_b.data_ptr(),
                                        ws.data_ptr(), nbytes, _stream()), "ufr_denoise_vertices")
    return dict(verts=_ring_result(pos_a, pos_b, n_vertex), normals=normals, border=border)


# ---- a scan loader's per-pixel work (csrc/frame_input.hip; uforecon_amd/dtu_scan.py is the caller)
def image_resize_u8(images: torch.Tensor, H: int, W: int, clip=(0, 0, 0, 0)) -> torch.Tensor:
    """ufr_image_resize_u8: (n,Hs,Ws,3) CUDA uint8 RGB -> (n,3,Ho,Wo) float32 planes in [0,1]: every image resized to ``H`` x
    ``W`` with OpenCV's 8-bit bilinear rule as include/ufr.h restates it (the 2x2 box mean when both factors are exactly 2),
    cropped by ``clip`` = (left, top, right, bottom) and divided by 255.  Does not synchronise."""
    p = _dev(images, "images", torch.uint8)
    if images.dim() != 4 or images.shape[3] != 3:
        raise UfrError(f"images: expected shape (n, Hs, Ws, 3), got {tuple(images.shape)}")
    clip = [int(c) for c in clip]
    if len(clip) != 4:
        raise UfrError(f"image_resize_u8: clip {clip!r} (left, top, right, bottom)")
    n, Hs, Ws = (int(s) for s in images.shape[:3])
    H, W = int(H), int(W)
    Ho, Wo = H - clip[1] - clip[3], W - clip[0] - clip[2]
    out = torch.empty((n, 3, max(Ho, 0), max(Wo, 0)), dtype=torch.float32, device=images.device)
    _lib.check(_lib.load().ufr_image_resize_u8(p, n, Hs, Ws, H, W, (C.c_int32 * 4)(*clip), out.data_ptr(), _stream()),
               "ufr_image_resize_u8")
    return out


def image_resize_mask_u8(images: torch.Tensor, masks: torch.Tensor, H: int, W: int, clip=(0, 0, 0, 0)) -> torch.Tensor:
    """ufr_image_resize_mask_u8: `image_resize_u8` with a foreground mask ``masks`` (n,Hs,Ws) CUDA uint8 that goes through the
    same resize; each output is float32((v / 255) * (m / 254)) in float64 (the reference's divisor).  Does not synchronise."""
    p = _dev(images, "images", torch.uint8)
    q = _dev(masks, "masks", torch.uint8)
    if images.dim() != 4 or images.shape[3] != 3 or tuple(masks.shape) != tuple(images.shape[:3]):
        raise UfrError(f"images / masks: expected shapes (n, Hs, Ws, 3) and (n, Hs, Ws), got {tuple(images.shape)} and {tuple(masks.shape)}")
    clip = [int(c) for c in clip]
    if len(clip) != 4:
        raise UfrError(f"image_resize_mask_u8: clip {clip!r} (left, top, right, bottom)")
    n, Hs, Ws = (int(s) for s in images.shape[:3])
    H, W = int(H), int(W)
    Ho, Wo = H - clip[1] - clip[3], W - clip[0] - clip[2]
    out = torch.empty((n, 3, max(Ho, 0), max(Wo, 0)), dtype=torch.float32, device=images.device)
    _lib.check(_lib.load().ufr_image_resize_mask_u8(p, q, n, Hs, Ws, H, W, (C.c_int32 * 4)(*clip), out.data_ptr(), _stream()),
               "ufr_image_resize_mask_u8")
    return out


def view_pair_scores(offsets, obs, points, centres, theta0: float = 5.0, sigma1: float = 1.0, sigma2: float = 10.0,
                     device="cuda") -> torch.Tensor:
    """ufr_view_pair_scores: the (N,N) float64 score matrix, on ``device``, of a COLMAP model's view selection.  ``offsets``
    (N+1) and ``obs`` (n_obs; -1 = no point) are the images' observation lists in CSR form, host arrays (``obs`` is uploaded
    here and also checked on the host); ``points`` (M,3) and ``centres`` (N,3) float64, host arrays or tensors on ``device``.
    Does not synchronise beyond torch's own uploads; uforecon_amd.colmap2mvsnet has the host form."""
    import numpy as np

    device = torch.device(device)
    if device.type != "cuda":
        raise UfrError(f"view_pair_scores: device {device} (must be a GPU; uforecon_amd.colmap2mvsnet has the host form)")
    off = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    ob = np.asarray(obs).reshape(-1)
    if ob.size and (ob.min() < -2 ** 31 or ob.max() >= 2 ** 31):
        raise UfrError("view_pair_scores: an observation index does not fit 32 bits")
    ob = np.ascontiguousarray(ob.astype(np.int32))
    N = off.size - 1
    lib = _lib.load()
    with torch.cuda.device(device):
        f64 = lambda t, name: (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float64)))).to(device)  # noqa: E731
        pts, cen = f64(points, "points").reshape(-1, 3), f64(centres, "centres")
        if cen.dim() != 2 or tuple(cen.shape) != (max(N, 0), 3):
            raise UfrError(f"view_pair_scores: centres {tuple(cen.shape)} for {N} images")
        nbytes = lib.ufr_view_pair_scores_workspace_bytes(N, ob.size)
        if nbytes == 0:
            raise UfrError("ufr_view_pair_scores failed (-1): " + lib.ufr_last_error().decode())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        ob_dev = torch.from_numpy(ob).to(device)
        out = torch.empty((N, N), dtype=torch.float64, device=device)
        _lib.check(lib.ufr_view_pair_scores(off.ctypes.data_as(C.POINTER(C.c_int64)), _dev(ob_dev, "obs", torch.int32) if ob.size else None,
                                            ob.ctypes.data_as(C.POINTER(C.c_int32)), ob.size,
                                            _dev(pts, "points", torch.float64) if pts.numel() else None, int(pts.shape[0]),
                                            _dev(cen, "centres", torch.float64), N, float(theta0), float(sigma1), float(sigma2),
                                            out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ufr_view_pair_scores")
    return out


def image_undistort_u8(src: torch.Tensor, model, params, k_out, H: int, W: int, want_valid: bool = True):
    """ufr_image_undistort_u8: (n,Hs,Ws,C) CUDA uint8 pictures of ONE COLMAP camera (C = 1 .. 4) -> ``(dst, valid)``: dst
    (n,H,W,C) uint8, the pictures as the pinhole camera ``k_out`` = (fx', fy', cx', cy') sees them, and valid (H,W) uint8, 255
    where an output pixel has a source and 0 where it does not (None without ``want_valid``).  ``model`` is COLMAP's model
    name or id, ``params`` that model's parameter list (host values).  The rule is stated in include/ufr.h;
    uforecon_amd.undistort has the host form.  Does not synchronise."""
    import numpy as np

    from .colmap2mvsnet import CAMERA_MODELS, MODEL_IDS

    p = _dev(src, "src", torch.uint8)
    if src.dim() != 4:
        raise UfrError(f"src: expected shape (n, Hs, Ws, C), got {tuple(src.shape)}")
    model_id = MODEL_IDS.get(model, -1) if isinstance(model, str) else int(model)
    par = np.ascontiguousarray(np.asarray(params, np.float64).reshape(-1))
    if model_id in CAMERA_MODELS and par.size != CAMERA_MODELS[model_id][1]:
        raise UfrError(f"image_undistort_u8: {par.size} parameters for camera model {CAMERA_MODELS[model_id][0]}, which has {CAMERA_MODELS[model_id][1]}")
    ko = np.ascontiguousarray(np.asarray(k_out, np.float64).reshape(-1))
    if ko.size != 4:
        raise UfrError(f"image_undistort_u8: k_out {tuple(np.shape(k_out))} (fx', fy', cx', cy')")
    n, Hs, Ws, Cn = (int(s) for s in src.shape)
    H, W = int(H), int(W)
    dst = torch.empty((n, max(H, 0), max(W, 0), Cn), dtype=torch.uint8, device=src.device)
    valid = torch.empty((max(H, 0), max(W, 0)), dtype=torch.uint8, device=src.device) if want_valid else None
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().ufr_image_undistort_u8(p, n, Hs, Ws, Cn, model_id, par.ctypes.data_as(dp), ko.ctypes.data_as(dp), H, W,
                                                  dst.data_ptr(), valid.data_ptr() if want_valid else None, _stream()),
               "ufr_image_undistort_u8")
    return dst, valid


def pixel_rays(m_inv, H: int, W: int, origin=None, device="cuda") -> torch.Tensor:
    """ufr_pixel_rays: (3,H*W) float32 unit vectors on ``device``; ``m_inv`` 4x4 and ``origin`` (3 values or None): host
    arrays, narrowed to float32.  Per pixel, in float64: p = (2x/(W-1) - 1, 2y/(H-1) - 1, 1, 1), v = (m_inv p)[:3] - origin,
    v / |v|.  Does not synchronise."""
    import numpy as np

    m = np.ascontiguousarray(np.asarray(m_inv, np.float32))
    if m.shape != (4, 4):
        raise UfrError(f"pixel_rays: m_inv {m.shape}: expected (4, 4)")
    fp = C.POINTER(C.c_float)
    po = None
    if origin is not None:
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(-1))
        if o.shape != (3,):
            raise UfrError(f"pixel_rays: origin {origin!r} (three values)")
        po = o.ctypes.data_as(fp)
    H, W = int(H), int(W)
    device = torch.device(device)
    if device.type != "cuda":
        raise UfrError(f"pixel_rays: device {device} (must be a GPU; uforecon_amd.dtu_scan has the host form)")
    with torch.cuda.device(device):
        out = torch.empty((3, max(H, 0) * max(W, 0)), dtype=torch.float32, device=device)
        _lib.check(_lib.load().ufr_pixel_rays(m.ctypes.data_as(fp), po, H, W, out.data_ptr(), _stream()), "ufr_pixel_rays")
    return out


def depth_gt_prepare(pfm_rows: torch.Tensor, bottom_up: bool, y0: int, x0: int, H: int, W: int, scale_factor: float,
                     cam_ray_z: torch.Tensor) -> torch.Tensor:
    """ufr_depth_gt_prepare: (H,W) float32 ground-truth ray depth of one training view from the (Hs,Ws) float32 rows of its PFM
    file as stored (``bottom_up``: the file's first row is the picture's last): nearest half-size picture, crop at (y0, x0),
    x ``scale_factor`` in float32, / ``cam_ray_z`` (H*W float64: row 2 of the float64 cam_ray_d) in float64.  Does not
    synchronise; uforecon_amd.dtu_train has the host form."""
    p = _dev(pfm_rows, "pfm_rows")
    if pfm_rows.dim() != 2:
        raise UfrError(f"pfm_rows: expected (Hs, Ws), got {tuple(pfm_rows.shape)}")
    H, W = int(H), int(W)
    z = _dev(cam_ray_z, "cam_ray_z", torch.float64)
    if cam_ray_z.numel() != max(H, 0) * max(W, 0):
        raise UfrError(f"cam_ray_z: {cam_ray_z.numel()} values for {H}x{W} pixels")
    out = torch.empty((max(H, 0), max(W, 0)), dtype=torch.float32, device=pfm_rows.device)
    _lib.check(_lib.load().ufr_depth_gt_prepare(p, int(pfm_rows.shape[0]), int(pfm_rows.shape[1]), int(bool(bottom_up)), int(y0), int(x0),
                                                H, W, float(scale_factor), z, out.data_ptr(), _stream()), "ufr_depth_gt_prepare")
    return out


CONV3D_S1, CONV3D_S2, CONV3D_T2 = 0, 1, 2


def conv3d(x_cl: torch.Tensor, weight: torch.Tensor, mode: int = CONV3D_S1, bias: Optional[torch.Tensor] = None,
           bn_scale: Optional[torch.Tensor] = None, bn_shift: Optional[torch.Tensor] = None, relu: bool = False,
           skip: Optional[torch.Tensor] = None, out_ncdhw: bool = False, weight2: Optional[torch.Tensor] = None,
           want_absmax: bool = False):
    """One 3x3x3 layer of the frustum U-Nets (ufr_conv3d).  ``want_absmax`` (channel-last outputs of at most 16 channels):
    returns ``(out, max |out| as a one-element device tensor)`` -- the bound a following plane layer wants.  ``x_cl`` (B,D,H,W,cin) channel-last; ``weight`` in the
    checkpoint's layout (conv (cout,cin,3,3,3); transposed conv, mode CONV3D_T2, (cin,cout,3,3,3)).  Returns the
    channel-last (B,Do,Ho,Wo,cout) output, or with ``out_ncdhw`` the reference's (B,cout,Do,Ho,Wo) -- and, when ``weight2``
    names a second head, the pair (out, sigmoid(second head))."""
    B, D, H, W, cin = x_cl.shape
    transposed = mode == CONV3D_T2
    cout = weight.shape[1] if transposed else weight.shape[0]
    if tuple(weight.shape) != ((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)):
        raise UfrError(f"conv3d: weight {tuple(weight.shape)} does not match {cin} input channels (mode {mode})")
    Do, Ho, Wo = ((2 * D, 2 * H, 2 * W) if transposed else ((D + 1) // 2, (H + 1) // 2, (W + 1) // 2) if mode == CONV3D_S2
                  else (D, H, W))
    dev = x_cl.device
    cout2 = 0 if weight2 is None else weight2.shape[0]
    out = torch.empty((B, cout, Do, Ho, Wo) if out_ncdhw else (B, Do, Ho, Wo, cout), dtype=torch.float32, device=dev)
    out2 = torch.empty((B, cout2, Do, Ho, Wo), dtype=torch.float32, device=dev) if cout2 else None
    if skip is not None and tuple(skip.shape) != tuple(out.shape):
        raise UfrError(f"conv3d: skip {tuple(skip.shape)} does not match the output {tuple(out.shape)}")
    keep = [t.detach().contiguous() for t in (weight, weight2, bias, bn_scale, bn_shift) if t is not None]
    it = iter(keep)
    ptr = lambda t, n: None if t is None else _dev(next(it), n)
    w_p, w2_p, b_p, s_p, h_p = ptr(weight, "weight"), ptr(weight2, "weight2"), ptr(bias, "bias"), ptr(bn_scale, "bn_scale"), \
        ptr(bn_shift, "bn_shift")
    # (want_absmax: True = a fresh zero word; or a caller-owned one-element ZERO tensor, e.g. a slice of a pool zeroed once)
    omax = want_absmax if isinstance(want_absmax, torch.Tensor) else (torch.zeros(1, dtype=torch.float32, device=dev) if want_absmax else None)
    _lib.check(_lib.load().ufr_conv3d(_dev(x_cl, "x"), w_p, w2_p, b_p, s_p, h_p, _opt(skip, "skip"), out.data_ptr(),
                                      _opt(out2, "out2"), B, D, H, W, cin, cout, cout2, int(mode), int(bool(relu)),
                                      int(bool(out_ncdhw)), _opt(omax, "out_absmax"), _stream()), "ufr_conv3d")
    if omax is not None:
        return out, omax
    return (out, out2) if cout2 else out


def absmax(x: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max |x| as a one-element device tensor (ufr_absmax: one pass at HBM speed, no host round trip); ``into``: a running
    maximum to raise instead of a fresh zero."""
    x = x.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    out = torch.zeros(1, dtype=torch.float32, device=x.device) if into is None else into
    _lib.check(_lib.load().ufr_absmax(_dev(x, "x"), x.numel(), out.data_ptr(), _stream()), "ufr_absmax")
    return out


# the weights' planes of ufr_conv3d_planes, kept while the weight TENSOR OBJECT lives unchanged: id(weight) -> (weak reference to
# it, its version counter, the same of weight2, flip, the planes).  Never keyed on an address: the allocator hands a freed
# tensor's address -- version 0 again -- to the next one.  An in-place update (optimizer.step) bumps the version, and the
# next call makes the planes again (training: once per layer and step; inference: once per checkpoint).
_PLANES = {}


def _planes_lookup(weight, weight2, flip, nbytes, transposed=False):
    import weakref

    ent = _PLANES.get(id(weight))
    sig = (weight._version, None if weight2 is None else (id(weight2), weight2._version), bool(flip), nbytes, weight.device, transposed)
    if ent is not None and ent[0]() is weight and ent[1] == sig and (weight2 is None or ent[2]() is weight2):
        return ent[3], True
    if len(_PLANES) > 512:          # tensors that died without being looked up again
        for k in [k for k, e in _PLANES.items() if e[0]() is None]:
            del _PLANES[k]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _PLANES[id(weight)] = (weakref.ref(weight), sig, None if weight2 is None else weakref.ref(weight2), ws)
    return ws, False


def conv3d_planes_supported(cin: int, cout: int, cout2: int = 0, mode: int = 0) -> bool:
    return _lib.load().ufr_conv3d_planes_workspace_bytes(cin, cout, cout2, int(mode)) > 0


def conv3d_planes(x_cl: torch.Tensor, x_absmax: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  bn_scale: Optional[torch.Tensor] = None, bn_shift: Optional[torch.Tensor] = None, relu: bool = False,
                  skip: Optional[torch.Tensor] = None, out_ncdhw: bool = False, weight2: Optional[torch.Tensor] = None,
                  flip: bool = False, want_absmax: bool = True, mode: int = 0):
    """A stride-1 3x3x3 layer with 8 or 16 input channels on the 16-bit matrix cores (ufr_conv3d_planes: fp16 plane
    products, fp32 accumulate, the input brick staged through LDS).  ``x_absmax``: one-element device tensor >= max |x_cl|
    (`absmax`, or the previous layer's returned bound).  ``flip``: the data gradient of a stride-1 layer -- ``weight`` is
    that layer's forward weight (cin of this call = its cout).  Returns ``(out, out_absmax or None)``, with a second head
    ``(out, sigmoid(out2), None)``."""
    B, D, H, W, cin = x_cl.shape
    if flip or int(mode) == CONV3D_T2:
        if tuple(weight.shape[2:]) != (3, 3, 3) or weight.shape[0] != cin:
            raise UfrError(f"conv3d_planes(flip / transposed): weight {tuple(weight.shape)} does not match {cin} input channels")
        cout = weight.shape[1]
    else:
        if tuple(weight.shape[1:]) != (cin, 3, 3, 3):
            raise UfrError(f"conv3d_planes: weight {tuple(weight.shape)} does not match {cin} input channels")
        cout = weight.shape[0]
    cout2 = 0 if weight2 is None else weight2.shape[0]
    lib = _lib.load()
    mode = int(mode)
    nbytes = lib.ufr_conv3d_planes_workspace_bytes(cin, cout, cout2, mode)
    if not nbytes:
        raise UfrError(f"conv3d_planes: (cin {cin}, cout {cout}+{cout2}, mode {mode}) is not a layer of this kernel family")
    dev = x_cl.device
    Do, Ho, Wo = ((D + 1) // 2, (H + 1) // 2, (W + 1) // 2) if mode == CONV3D_S2 else (2 * D, 2 * H, 2 * W) if mode == CONV3D_T2 else (D, H, W)
    out = torch.empty((B, cout, Do, Ho, Wo) if out_ncdhw else (B, Do, Ho, Wo, cout), dtype=torch.float32, device=dev)
    out2 = torch.empty((B, cout2, Do, Ho, Wo), dtype=torch.float32, device=dev) if cout2 else None
    if skip is not None and tuple(skip.shape) != tuple(out.shape):
        raise UfrError(f"conv3d_planes: skip {tuple(skip.shape)} does not match the output {tuple(out.shape)}")
    ws, ready = _planes_lookup(weight, weight2, flip, nbytes, mode == CONV3D_T2)
    omax = None
    if not out_ncdhw:
        omax = want_absmax if isinstance(want_absmax, torch.Tensor) else (torch.zeros(1, dtype=torch.float32, device=dev) if want_absmax else None)
    keep = [t.detach().contiguous() for t in (weight, weight2, bias, bn_scale, bn_shift) if t is not None]
    it = iter(keep)
    ptr = lambda t, n: None if t is None else _dev(next(it), n)
    w_p, w2_p, b_p, s_p, h_p = ptr(weight, "weight"), ptr(weight2, "weight2"), ptr(bias, "bias"), ptr(bn_scale, "bn_scale"), \
        ptr(bn_shift, "bn_shift")
    _lib.check(lib.ufr_conv3d_planes(_dev(x_cl, "x"), _dev(x_absmax, "x_absmax"), w_p, w2_p, b_p, s_p, h_p, _opt(skip, "skip"),
                                     out.data_ptr(), _opt(out2, "out2"), _opt(omax, "out_absmax"), B, D, H, W, cin, cout, cout2,
                                     mode, int(bool(relu)), int(bool(out_ncdhw)), int(bool(flip)), ws.data_ptr(), nbytes, int(ready),
                                     _stream()),
               "ufr_conv3d_planes")
    return (out, out2, None) if cout2 else (out, omax)


CONV2D_RELU, CONV2D_IN_PLANAR, CONV2D_OUT_PLANAR = 1, 2, 4


def conv2d(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, scale: Optional[torch.Tensor] = None,
           shift: Optional[torch.Tensor] = None, relu: bool = False, skip: Optional[torch.Tensor] = None,
           in_planar: bool = False, out_planar: bool = False, sigmoid_from: int = -1):
    """One plain convolution of FeatureNet (ufr_conv2d): ``x`` channel-last (B,H,W,cin) -- or, with ``in_planar``, the image
    (B,3,H,W); ``weight`` (cout,cin,k,k), zero padding k // 2; ``out = [relu](conv * scale + shift) [+ up2(skip)]``; returns
    channel-last (B,Ho,Wo,cout) or with ``out_planar`` (B,cout,Ho,Wo); ``sigmoid_from``: sigmoid on channels >= it."""
    if in_planar:
        B, cin, H, W = x.shape
    else:
        B, H, W, cin = x.shape
    cout, cin_w, k, k2 = weight.shape
    if cin_w != cin or k != k2:
        raise UfrError(f"conv2d: weight {tuple(weight.shape)} does not match {cin} input channels")
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    out = torch.empty((B, cout, Ho, Wo) if out_planar else (B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    if skip is not None and tuple(skip.shape) != (B, Ho // 2, Wo // 2, cout):
        raise UfrError(f"conv2d: skip {tuple(skip.shape)} is not the half-resolution map {(B, Ho // 2, Wo // 2, cout)}")
    flags = (CONV2D_RELU if relu else 0) | (CONV2D_IN_PLANAR if in_planar else 0) | (CONV2D_OUT_PLANAR if out_planar else 0)
    _lib.check(_lib.load().ufr_conv2d(_dev(x, "x"), _dev(weight, "weight"), _opt(scale, "scale"), _opt(shift, "shift"),
                                      _opt(skip, "skip"), out.data_ptr(), B, cin, cout, H, W, k, int(stride), flags,
                                      int(sigmoid_from), _stream()), "ufr_conv2d")
    return out


def upsample_add(reduced_cl: torch.Tensor, fine: torch.Tensor) -> torch.Tensor:
    """``bilinear_2x(reduced_cl (B,h,w,C)) + fine (B,C,2h,2w)`` -> channel-last (B,2h,2w,C) (ufr_upsample_add: the sum the
    smoothing convolutions of the FMT pathway read)."""
    B, h, w, Cc = reduced_cl.shape
    if tuple(fine.shape) != (B, Cc, 2 * h, 2 * w):
        raise UfrError(f"upsample_add: fine {tuple(fine.shape)} is not (B,C,2h,2w) of reduced {tuple(reduced_cl.shape)}")
    out = torch.empty(B, 2 * h, 2 * w, Cc, dtype=torch.float32, device=fine.device)
    _lib.check(_lib.load().ufr_upsample_add(_dev(reduced_cl, "reduced"), _dev(fine, "fine"), out.data_ptr(), B, Cc, h, w, _stream()),
               "ufr_upsample_add")
    return out


def deform_conv2d_cl(x_cl: torch.Tensor, offset_mask: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, relu: bool = False,
                     out_planar: bool = False):
    """The deformable 3x3 layer on a channel-last input (ufr_deform_conv2d_cl): ``x_cl`` (B,H,W,32); ``offset_mask``
    (B,27,H,W) planar = DCN.conv_offset_mask's output with the sigmoid already on channels 18..26 (``conv2d(...,
    out_planar=True, sigmoid_from=18)``); ``out = [relu]((dcn + bias) * scale + shift)``, channel-last or planar."""
    B, H, W, C = x_cl.shape
    Cout = weight.shape[0]
    if tuple(offset_mask.shape) != (B, 27, H, W) or tuple(weight.shape) != (Cout, C, 3, 3):
        raise UfrError(f"deform_conv2d_cl: shapes {tuple(x_cl.shape)} {tuple(offset_mask.shape)} {tuple(weight.shape)}")
    out = torch.empty((B, Cout, H, W) if out_planar else (B, H, W, Cout), dtype=torch.float32, device=x_cl.device)
    flags = (CONV2D_RELU if relu else 0) | (CONV2D_OUT_PLANAR if out_planar else 0)
    _lib.check(_lib.load().ufr_deform_conv2d_cl(_dev(x_cl, "x"), _dev(offset_mask, "offset_mask"), _dev(weight, "weight"),
                                                _opt(bias, "bias"), _opt(scale, "scale"), _opt(shift, "shift"), out.data_ptr(),
                                                B, C, Cout, H, W, flags, _stream()), "ufr_deform_conv2d_cl")
    return out


def conv3d_bwd_data(d_out_cl: torch.Tensor, weight: torch.Tensor, mode: int, in_shape, accumulate: Optional[torch.Tensor] = None):
    """Data gradient of one plain 3x3x3 layer (ufr_conv3d_bwd_data): ``d_out_cl`` channel-last at the layer's output extent,
    ``weight`` the layer's forward weight in the checkpoint's layout, ``in_shape`` = (B,D,H,W,cin) of the layer's input.
    ``accumulate`` (same shape): added -- a gradient arriving on two paths (the U-Net's skip additions)."""
    B, D, H, W, cin = in_shape
    cout = d_out_cl.shape[-1]
    d_in = torch.empty(in_shape, dtype=torch.float32, device=d_out_cl.device)
    w = weight.detach().contiguous()
    _lib.check(_lib.load().ufr_conv3d_bwd_data(_dev(d_out_cl, "d_out"), _dev(w, "weight"), _opt(accumulate, "accumulate"),
                                               d_in.data_ptr(), B, D, H, W, cin, cout, int(mode), _stream()), "ufr_conv3d_bwd_data")
    return d_in


def conv3d_bwd_weight_heads(x_cl: torch.Tensor, d_out_cl: torch.Tensor, d_out2_cl: torch.Tensor, out=None):
    """Weight gradients of CostRegNetWeight's two heads in one pass over the shared input (ufr_conv3d_bwd_weight_heads):
    ``x_cl`` (B,D,H,W,8), ``d_out_cl`` (B,D,H,W,8), ``d_out2_cl`` (B,D,H,W,1) -> (d features.weight (8,8,3,3,3),
    d weights.weight (1,8,3,3,3))."""
    B, D, H, W, cin = x_cl.shape
    if cin != 8 or tuple(d_out_cl.shape) != (B, D, H, W, 8) or tuple(d_out2_cl.shape) != (B, D, H, W, 1):
        raise UfrError(f"conv3d_bwd_weight_heads: shapes {tuple(x_cl.shape)}, {tuple(d_out_cl.shape)}, {tuple(d_out2_cl.shape)}")
    # out = (dw, dw2): caller-owned ZEROED tensors of those shapes (slices of one buffer zeroed once per backward)
    dw, dw2 = out if out is not None else (torch.zeros(8, 8, 3, 3, 3, dtype=torch.float32, device=x_cl.device),
                                           torch.zeros(1, 8, 3, 3, 3, dtype=torch.float32, device=x_cl.device))
    _lib.check(_lib.load().ufr_conv3d_bwd_weight_heads(_dev(x_cl, "in"), _dev(d_out_cl, "d_out"), _dev(d_out2_cl, "d_out2"), dw.data_ptr(),
                                                       dw2.data_ptr(), B, D, H, W, _stream()), "ufr_conv3d_bwd_weight_heads")
    return dw, dw2


def conv3d_bwd_weight(x_cl: torch.Tensor, d_out_cl: torch.Tensor, mode: int, weight_shape, want_bias: bool = True, out=None):
    """Weight (and bias) gradient of one plain 3x3x3 layer (ufr_conv3d_bwd_weight) -> (d_weight in the checkpoint's
    layout, d_bias or None)."""
    B, D, H, W, cin = x_cl.shape
    cout = d_out_cl.shape[-1]
    if out is not None:      # (dw, db): caller-owned ZEROED tensors (slices of one buffer zeroed once per backward)
        dw, db = out
    else:
        dw = torch.zeros(weight_shape, dtype=torch.float32, device=x_cl.device)
        db = torch.zeros(cout, dtype=torch.float32, device=x_cl.device) if want_bias else None
    _lib.check(_lib.load().ufr_conv3d_bwd_weight(_dev(x_cl, "in"), _dev(d_out_cl, "d_out"), dw.data_ptr(), _opt(db, "d_bias"),
                                                 B, D, H, W, cin, cout, int(mode), _stream()), "ufr_conv3d_bwd_weight")
    return dw, db



# ---------------------------------------------------------------- the optimizer update and the ray draw of a training step
def adam_table_capacity() -> int:
    """Tensors one launch of ufr_adam_step carries (UFR_ADAM_TABLE_CAPACITY)."""
    return int(_lib.load().ufr_adam_table_capacity())


@torch.no_grad()
def adam_step(params, grads, exp_avgs, exp_avg_sqs, bias_corrections1, bias_corrections2, lr: float, beta1: float = 0.9,
              beta2: float = 0.999, eps: float = 1e-8) -> None:
    """torch.optim.Adam's update with its defaults for a list of fp32 tensors, in place: ufr_adam_step (one launch per
    ``adam_table_capacity()`` tensors) on the GPU; on CPU tensors the same formula as torch expressions -- the statement of
    what the kernel computes.  ``bias_corrections1 / 2``: per tensor 1 - beta^step of ITS step count, python floats.  The
    kernel writes through raw pointers, so the version counters of the tensors it changed are advanced here: caches keyed on
    them (RayTransformer.packed_weights, the convolutions' weight planes) and autograd's saved-tensor check see the update."""
    import math

    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(bias_corrections1) == len(bias_corrections2) == n):
        raise UfrError("adam_step: the six lists differ in length")
    if n == 0:
        return
    if not params[0].is_cuda:
        for p, g, m, v, bc1, bc2 in zip(params, grads, exp_avgs, exp_avg_sqs, bias_corrections1, bias_corrections2):
            if p.is_cuda or p.dtype != torch.float32:
                raise UfrError("adam_step: fp32 tensors, all on the CPU or all on the GPU")
            m.add_((g - m) * (1.0 - beta1))
            v.mul_(beta2).add_(g * g * (1.0 - beta2))
            p.sub_((lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)))
        return
    AdamTable(params, exp_avgs, exp_avg_sqs).step(grads, bias_corrections1, bias_corrections2, lr, beta1, beta2, eps)


class AdamTable:
    """The ufr_adam_tensor table of a fixed set of GPU tensors (parameter, exp_avg, exp_avg_sq), checked and filled once: a
    step then sets the gradients' addresses and the bias corrections and makes the call -- the host's share of an optimizer
    step is most of it (~62 small tensors).  Holds the tensors, so none of the addresses it recorded can be handed to another
    allocation; `current()` says whether the parameters still live where they did (`.to()`, `p.data = ...` move them)."""

    def __init__(self, params, exp_avgs, exp_avg_sqs):
        n = len(params)
        if not (len(exp_avgs) == len(exp_avg_sqs) == n):
            raise UfrError("adam_step: the lists differ in length")
        self.params = list(params)
        self.tensors = self.params + list(exp_avgs) + list(exp_avg_sqs)
        self.table = (_lib.AdamTensor * n)()
        self.rows = list(self.table)           # views of the table's rows
        for i, (e, p, m, v) in enumerate(zip(self.rows, params, exp_avgs, exp_avg_sqs)):
            if m.shape != p.shape or v.shape != p.shape:
                raise UfrError(f"adam_step: tensor {i}: parameter {tuple(p.shape)}, state {tuple(m.shape)} {tuple(v.shape)}")
            e.param, e.exp_avg, e.exp_avg_sq, e.numel = _dev(p, "param"), _dev(m, "exp_avg"), _dev(v, "exp_avg_sq"), p.numel()
        self.param_ptrs = [p.data_ptr() for p in self.params]

    def current(self) -> bool:
        return self.param_ptrs == [p.data_ptr() for p in self.params]

    @torch.no_grad()
    def step(self, grads, bias_corrections1, bias_corrections2, lr: float, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8) -> None:
        n = len(self.rows)
        if not (len(grads) == len(bias_corrections1) == len(bias_corrections2) == n):
            raise UfrError("adam_step: the lists differ in length")
        if n == 0:
            return
        keep = []
        for e, p, g, b1, b2 in zip(self.rows, self.params, grads, bias_corrections1, bias_corrections2):
            if g.shape != p.shape:
                raise UfrError(f"adam_step: parameter {tuple(p.shape)}, gradient {tuple(g.shape)}")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            e.grad, e.bias_correction1, e.bias_correction2 = _dev(g, "grad"), b1, b2
        _lib.check(_lib.load().ufr_adam_step(self.table, n, float(lr), float(beta1), float(beta2), float(eps), _stream()), "ufr_adam_step")
        torch.autograd.graph.increment_version(self.tensors)


def select_rays(u: torch.Tensor, k: int) -> torch.Tensor:
    """The first ``k`` entries of the stable ascending argsort of the 1-D fp32 tensor ``u`` (int64): model.py:537's
    ``argsort(rand(H W))[:train_ray_num]`` with equal values in index order.  GPU: ufr_select_rays (1 <= k <= min(n, 4096),
    n <= 2^24; no synchronisation); CPU: ``torch.sort(stable=True)``, the statement of what the kernels compute."""
    if not isinstance(u, torch.Tensor) or u.dim() != 1 or u.dtype != torch.float32:
        raise UfrError("select_rays: u must be a 1-D float32 tensor")
    n, k = u.numel(), int(k)
    if not u.is_cuda:
        if not 1 <= k <= n:
            raise UfrError(f"select_rays: k={k} with n={n} (1 <= k <= n)")
        return torch.sort(u, stable=True).indices[:k]
    lib = _lib.load()
    if n > 2 ** 31 - 1:
        raise UfrError(f"select_rays: n={n}")
    nbytes = lib.ufr_select_rays_workspace_bytes(n, k)
    if nbytes == 0:
        raise UfrError("ufr_select_rays failed (-1): " + lib.ufr_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=u.device)
    out = torch.empty(k, dtype=torch.int64, device=u.device)
    _lib.check(lib.ufr_select_rays(_dev(u, "u"), n, k, out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ufr_select_rays")
    return out
