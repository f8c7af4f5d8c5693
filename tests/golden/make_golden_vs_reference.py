"""Golden vectors of the three checks that used to import the reference at test time, by RUNNING THE REFERENCE (CPU,
build container only):  ``python tests/golden/make_golden_vs_reference.py`` -> tests/golden/vs_reference.npz.

Both ray-path runs load the committed seed-0 weights (tests/golden/ray_path_weights_seed0.npz) into the reference model:
* ``infer/*``: the reference's ``UFORecon.infer`` (extract_geometry) on 12 rays of ``make_frame(32, 48, 3, seed=21)``,
  32 + 32 samples, uniforms from ``torch.manual_seed(4)`` (= ``sampler_uniforms(4, ...)``).
* ``train/*``: one training forward of the reference (train mode) on 10 rays of ``make_frame(32, 48, 3, seed=22,
  train_layout=True)`` after ``torch.manual_seed(5)``, ``oracle.training_loss`` of its outputs and the ray-path parameter
  gradients of that loss through the reference's autograd.
* ``fnet/*``: the reference FeatureNet(8) filled by ``fill_state_dict(..., 11)``: its state_dict keys, the repr of the
  plain-convolution trunk (conv0 / conv1 / conv2 / inner2) and what that trunk computes on a seeded image.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

from ref_harness import build_reference_model, import_reference  # noqa: E402
from oracle import ufo_oracle as O  # noqa: E402
from uforecon_amd.scene import fill_state_dict, make_frame  # noqa: E402

OUT = os.path.join(HERE, "vs_reference.npz")
TRUNK = ("conv0", "conv1", "conv2", "inner2")


def _with_weights(model, P):
    missing, unexpected = model.load_state_dict(P, strict=False)
    assert not unexpected and not any(k in P for k in missing)
    return model


def main():
    g = {}
    wz = np.load(os.path.join(HERE, "ray_path_weights_seed0.npz"))
    P = {k: torch.from_numpy(wz[k]) for k in wz.files}
    # inference (tests/test_oracle_vs_reference.py::test_infer_matches_the_imported_reference)
    model = build_reference_model(0, test_sample_coarse=32, test_sample_fine=32, coarse_sample=32, fine_sample=32, test_n_view=3)
    model = _with_weights(model, P)
    fr = make_frame(32, 48, 3, seed=21)
    idx = (torch.arange(12) * 100 + 57)[None]
    with torch.no_grad():
        torch.manual_seed(4)
        srdf, pts, depth, rgb = model.infer(batch=fr.batch, ray_idx=idx, source_imgs_feat=fr.source_imgs_feat,
                                            feature_volume=fr.feature_volume, match_feature=fr.match_feature,
                                            extract_geometry=True, is_train=False)
    for k, v in dict(srdf=srdf, pts=pts, depth=depth, rgb=rgb).items():
        g[f"infer/{k}"] = v[0].numpy()

    # training (tests/test_oracle_vs_reference.py::test_training_gradients_match_the_imported_reference)
    model = _with_weights(build_reference_model(0, test_sample_coarse=32, test_sample_fine=32, coarse_sample=32, fine_sample=32,
                                                test_n_view=3, extract_geometry=False), P)
    model.train()
    fr = make_frame(32, 48, 3, seed=22, train_layout=True)
    idx = (torch.arange(10) * 120 + 250)[None]
    torch.manual_seed(5)
    r = model.infer(batch=fr.batch, ray_idx=idx, source_imgs_feat=fr.source_imgs_feat, feature_volume=fr.feature_volume,
                    match_feature=fr.match_feature)
    loss = O.training_loss(dict(rgb=r[1][0], depth=r[2][0], rgb_2=r[8][0], depth_2=r[9][0]), fr.batch, idx)
    loss.backward()
    g["train/loss"] = np.array(float(loss), dtype=np.float64)
    for k, p in model.named_parameters():
        if k in P and p.grad is not None:
            g[f"train/grad/{k}"] = p.grad.numpy()

    # FeatureNet trunk (tests/test_dcn.py::test_mirror_keys_and_plain_convolutions_match_the_reference)
    import_reference()
    from code1.encoder_utils.fmt.module import FeatureNet as Ref

    ref = fill_state_dict(Ref(base_channels=8), 11).eval()
    g["fnet/keys"] = np.array(sorted(ref.state_dict()))
    for n in TRUNK:
        g[f"fnet/repr/{n}"] = np.array(repr(getattr(ref, n)))
    x = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        for n in ("conv0", "conv1", "conv2"):
            x = getattr(ref, n)(x)
            g[f"fnet/{n}"] = x.numpy()
        g["fnet/inner2_conv0_ones"] = ref.inner2(ref.conv0(torch.ones(1, 3, 8, 8))).numpy()
    np.savez_compressed(OUT, **g)
    print(OUT, os.path.getsize(OUT), "bytes,", len(g), "arrays")


if __name__ == "__main__":
    main()
