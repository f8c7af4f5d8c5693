"""ufr_render_rays_pair: both passes of the fused ray path.  Its fine outputs are ufr_render_rays' bits, its coarse outputs
the bits of a coarse_only render with the same uniforms, and without cam_ray_d (near/far as given, model.py:423) all four
are the oracle's infer(extract_geometry=False) within the north-star tolerance of tests/test_gpu_parity.py."""
import pytest
import torch

from helpers import REL_TOL, border_degenerate_rays, load_weights, max_rel_elem
from oracle import ufo_oracle as O
from uforecon_amd import ops
from uforecon_amd._lib import UfrError
from uforecon_amd.scene import make_frame, sampler_uniforms

DEV = "cuda:0"
H, W = 48, 64
# name -> views, frame seed, rays, coarse + fine samples, sampler seed, chunk (0: the default), side streams
CASES = {
    "nv2": dict(NV=2, seed=22, RN=24, SN=64, PN=64, useed=3),
    "nv3": dict(NV=3, seed=23, RN=24, SN=64, PN=64, useed=4),
    "nv7": dict(NV=7, seed=27, RN=24, SN=64, PN=64, useed=5),
    "s64_32": dict(NV=3, seed=31, RN=24, SN=64, PN=32, useed=6),          # 96 samples: the sequence-length division is a true one
    "ragged_chunks": dict(NV=3, seed=33, RN=150, SN=64, PN=64, useed=7, chunk=64, streams=3),     # 64 + 64 + 22 rays, side streams
    "ragged_chunks_one_stream": dict(NV=3, seed=33, RN=150, SN=64, PN=64, useed=7, chunk=64, streams=1),
}


def case_inputs(name):
    c = CASES[name]
    fr = make_frame(H, W, c["NV"], seed=c["seed"], train_layout=True)
    step = (H * W - 40) // c["RN"]
    idx = (torch.arange(c["RN"]) * step + 37)[None]
    U1, U2 = sampler_uniforms(c["useed"], c["SN"], c["PN"], c["RN"])
    return c, fr, idx, U1, U2


def oracle_both_passes(name):
    c, fr, idx, U1, U2 = case_inputs(name)
    want = {}
    with torch.no_grad():
        r = O.infer(load_weights(), fr.batch, idx, fr.source_imgs_feat, fr.feature_volume, fr.match_feature, U1, U2,
                    extract_geometry=False, want=want)
    return r, want


@pytest.mark.parametrize("name", list(CASES))
def test_border_exclusion_stays_small(name):
    """(CPU) the rays whose RGB the parity check leaves out -- a sample ON a source-image border, where the reference's mask is
    a step function of the last ulp (tests/test_gpu_parity.py) -- are under a quarter of each case's rays, in both passes."""
    _, want = oracle_both_passes(name)
    for tag in ("coarse", "fine"):
        frac = float(border_degenerate_rays(want[tag]).float().mean())
        print(f"{name} {tag}: {frac:.1%} of the rays excluded")
        assert frac < 0.25


@pytest.fixture(scope="module")
def weights():
    return ops.PackedWeights({k: v.to(DEV) for k, v in load_weights().items()})


def _handle(fr, drop=()):
    f = fr.to(DEV)
    return ops.FrameHandle({k: v for k, v in f.batch.items() if k not in drop}, f.source_imgs_feat, f.feature_volume, f.match_feature)


def _workspace(c):
    if not c.get("chunk"):
        return None
    return ops.RenderWorkspace(DEV, c["SN"], c["PN"], c["NV"], chunk_rays=c["chunk"], n_streams=c["streams"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pair_is_render_rays_plus_the_coarse_pass(name, weights):
    c, fr, idx, U1, U2 = case_inputs(name)
    fh = _handle(fr)
    i, u1, u2 = idx.reshape(-1).to(DEV), U1.to(DEV), U2.to(DEV)
    pair = ops.render_rays(fh, weights, i, u1, u2, workspace=_workspace(c), pair=True)
    plain = ops.render_rays(fh, weights, i, u1, u2, workspace=_workspace(c))
    for k in ("rgb", "depth", "depth_z", "srdf", "z_all"):
        assert torch.equal(pair[k], plain[k]), k
    ws = ops.RenderWorkspace(DEV, c["SN"], 0, c["NV"], chunk_rays=c["chunk"], n_streams=c["streams"]) if c.get("chunk") else None
    coarse = ops.render_rays(fh, weights, i, u1, None, coarse_only=True, workspace=ws)
    assert torch.equal(pair["rgb_coarse"], coarse["rgb"])
    assert torch.equal(pair["depth_coarse"], coarse["depth"])
    assert tuple(pair["rgb_coarse"].shape) == (c["RN"], 3) and tuple(pair["depth_coarse"].shape) == (c["RN"],)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pair_without_cam_ray_d_is_the_validation_signature(name, weights):
    c, fr, idx, U1, U2 = case_inputs(name)
    r, want = oracle_both_passes(name)
    fh = _handle(fr, drop=("cam_ray_d",))
    out = ops.render_rays(fh, weights, idx.reshape(-1).to(DEV), U1.to(DEV), U2.to(DEV), workspace=_workspace(c), pair=True)
    assert out["depth_z"] is None
    for tag, rgb, depth, rgb_ref, depth_ref in (("coarse", out["rgb_coarse"], out["depth_coarse"], r["rgb"], r["depth"]),
                                                ("fine", out["rgb"], out["depth"], r["rgb_2"], r["depth_2"])):
        assert max_rel_elem(depth, depth_ref.reshape(-1), floor=1e-3) < REL_TOL, tag
        ok = ~border_degenerate_rays(want[tag])
        assert max_rel_elem(rgb[ok.to(DEV)], rgb_ref.reshape(-1, 3)[ok], floor=0.05) < REL_TOL, tag


@pytest.mark.gpu
def test_pair_refusals(weights):
    import ctypes as C

    from uforecon_amd import _lib

    c, fr, idx, U1, U2 = case_inputs("nv3")
    i, u1, u2 = idx.reshape(-1).to(DEV), U1.to(DEV), U2.to(DEV)
    with pytest.raises(UfrError, match="coarse_only"):
        ops.render_rays(_handle(fr), weights, i, u1, None, coarse_only=True, pair=True)
    with pytest.raises(UfrError, match="cam_ray_d"):            # the requirement is lifted on the pair route only
        ops.render_rays(_handle(fr, drop=("cam_ray_d",)), weights, i, u1, u2)
    # the C entry itself: coarse_only, and depth_z without cam_ray_d
    fh = _handle(fr)
    ws = ops.RenderWorkspace(DEV, c["SN"], c["PN"], c["NV"])
    RN = c["RN"]
    depth, rgb = torch.empty(RN, device=DEV), torch.empty(RN, 3, device=DEV)
    depth_c, rgb_c, depth_z = torch.empty(RN, device=DEV), torch.empty(RN, 3, device=DEV), torch.empty(RN, device=DEV)
    a = _lib.RenderArgs()
    a.frame, a.packed_weights, a.raw = C.pointer(fh.frame), weights.packed.data_ptr(), C.pointer(weights.raw)
    a.ray_idx, a.ray_d, a.cam_ray_d = i.data_ptr(), fh.ray_d.data_ptr(), fh.cam_ray_d.data_ptr()
    a.ray_o = (C.c_float * 3)(*fh.ray_o)
    a.near_z, a.far_z = fh.near_z, fh.far_z
    a.U1, a.U2 = u1.data_ptr(), u2.data_ptr()
    a.RN, a.SN, a.PN, a.coarse_only, a.precision = RN, c["SN"], c["PN"], 0, weights.mode()
    a.depth, a.rgb, a.depth_z = depth.data_ptr(), rgb.data_ptr(), depth_z.data_ptr()
    a.chunk_rays, a.n_streams, a.workspace, a.workspace_bytes = ws.chunk, ws.n_streams, ws.buf.data_ptr(), ws.nbytes
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.ufr_render_rays_pair(C.byref(a), rgb_c.data_ptr(), depth_c.data_ptr(), s) == 0
    assert lib.ufr_render_rays_pair(C.byref(a), None, depth_c.data_ptr(), s) == -1
    a.coarse_only = 1
    assert lib.ufr_render_rays_pair(C.byref(a), rgb_c.data_ptr(), depth_c.data_ptr(), s) == -1
    assert b"coarse_only" in lib.ufr_last_error()
    a.coarse_only, a.cam_ray_d = 0, None
    assert lib.ufr_render_rays_pair(C.byref(a), rgb_c.data_ptr(), depth_c.data_ptr(), s) == -1
    assert b"depth_z" in lib.ufr_last_error()
    a.depth_z = None
    assert lib.ufr_render_rays_pair(C.byref(a), rgb_c.data_ptr(), depth_c.data_ptr(), s) == 0
    torch.cuda.synchronize()
