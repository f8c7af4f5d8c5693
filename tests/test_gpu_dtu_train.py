"""DtuTrain(device="cuda:0") against DtuTrain(device="cpu") on the synthetic training tree of tests/dtu_train_golden.py: the
host-side entries are the same code; the per-pixel ones come from the kernels (pictures and ground-truth depths exact, ray_d within
the bound tests/test_gpu_dtu_scan.py derives for ufr_pixel_rays against its host form)."""
import numpy as np
import pytest
import torch

import dtu_train_golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAY_ATOL = 1.2e-7          # tests/test_gpu_dtu_scan.py: one float32 step of a unit vector's component (the kernel sums in another order)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return G.write_tree(tmp_path_factory.mktemp("dtu_train_gpu"))


@pytest.mark.parametrize("case,i", [("test", 4), ("train", 275)])
def test_device_batch_equals_host_batch(tree, case, i):
    host = G.flat_batch(G.open_dataset(tree, case, "cpu")[i])
    batch = G.open_dataset(tree, case, DEV)[i]
    assert all(t.device == torch.device(DEV) for k, t in batch.items() if torch.is_tensor(t))
    assert all(t.device == torch.device(DEV) for t in batch["proj_matrices"].values())
    dev = G.flat_batch(batch)
    assert set(dev) == set(host)
    for k, w in host.items():
        if k == "meta":
            assert dev[k] == w
            continue
        assert dev[k].shape == w.shape and dev[k].dtype == w.dtype, k
        if k == "ray_d":
            assert np.abs(dev[k].astype(np.float64) - w).max() <= RAY_ATOL, k
        else:
            assert np.array_equal(dev[k], w), k                    # images, depths_h (holes included) and every camera entry
    assert (host["depths_h"] == 0).any() and (host["depths_h"] != 0).any()
