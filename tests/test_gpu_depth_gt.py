"""ufr_depth_gt_prepare (csrc/frame_input.hip) against its host form (uforecon_amd.dtu_train.depth_gt_host), bit for bit."""
import numpy as np
import pytest
import torch

from uforecon_amd import _lib, ops
from uforecon_amd.dtu_train import depth_gt_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _source(Hs, Ws, seed):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(250, 1250, (Hs, Ws)).astype(np.float32)
    rows[rng.uniform(size=rows.shape) < 0.25] = 0.0              # holes
    return rows


# source size, crop (y0, x0, H, W): an even source with an interior crop; an odd one (25 -> 12 rows, 41 -> 20 columns) cropped to
# its last half-size row and column; 27 x 43 -> 14 x 22 (half to even rounds up): the whole half-size picture, more than one block
@pytest.mark.parametrize("Hs,Ws,crop", [(24, 40, (2, 3, 8, 12)), (25, 41, (4, 8, 8, 12)), (27, 43, (0, 0, 14, 22))])
@pytest.mark.parametrize("bottom_up", [True, False])
def test_equals_the_host_form(Hs, Ws, crop, bottom_up):
    y0, x0, H, W = crop
    rows = _source(Hs, Ws, Hs + Ws)
    z = np.random.default_rng(1).uniform(0.8, 1.0, H * W)           # float64, as the reference's cam_ray_d
    sf = float(np.float32(1.0 / 320.7))
    want = depth_gt_host(rows, bottom_up, y0, x0, H, W, sf, z)
    got = ops.depth_gt_prepare(torch.from_numpy(rows).to(DEV), bottom_up, y0, x0, H, W, sf, torch.from_numpy(z).to(DEV)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (H, W)
    assert np.array_equal(got, want)
    picture = np.flipud(rows) if bottom_up else rows
    assert np.array_equal(got == 0, picture[0::2, 0::2][y0:y0 + H, x0:x0 + W] == 0) and (got == 0).any() and (got != 0).any()


def test_argument_errors():
    lib = _lib.load()
    rows = torch.zeros(24, 40, device=DEV)
    z = torch.ones(8 * 12, dtype=torch.float64, device=DEV)
    out = torch.zeros(8, 12, device=DEV)
    p, q, o = rows.data_ptr(), z.data_ptr(), out.data_ptr()
    ok = (p, 24, 40, 1, 2, 3, 8, 12, 1.0, q, o, None)

    def call(**kw):
        names = ("pfm", "Hs", "Ws", "bottom_up", "y0", "x0", "H", "W", "scale", "z", "depth", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.ufr_depth_gt_prepare(*[a[n] for n in names])

    assert call() == 0
    for bad in (dict(pfm=None), dict(z=None), dict(depth=None), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(bottom_up=2),
                dict(y0=-1), dict(x0=-1), dict(y0=5), dict(x0=9), dict(H=13), dict(W=21), dict(z=q + 4)):
        assert call(**bad) == -1, bad
        assert lib.ufr_last_error()
    torch.cuda.synchronize()
    with pytest.raises(_lib.UfrError):
        ops.depth_gt_prepare(rows, True, 2, 3, 8, 12, 1.0, z[:-1])
