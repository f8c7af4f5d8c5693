"""The CPU oracle reproduces the reference's golden vectors (CPU-only test).

Pins oracle/ufo_oracle.py against outputs of the reference itself (tests/golden/*.npz,
made by tests/golden/make_golden.py from /root/reference).
"""
import os

import pytest
import torch

from helpers import CASES, REL_TOL, case_inputs, case_weights, load_weights, rel_err
from oracle import ufo_oracle as O

EXACT = 2e-6  # oracle vs reference differ only by op-order rounding


@pytest.mark.parametrize("name", ["c1_coarse_only", "c2_hier_small", "c4_nv5_128", "c2_hier_512x640", "c2_hier_interior",
                                  "c4_nv5_interior", "c2_hier_512x640_interior"])
def test_infer_matches_reference_golden(name):
    c = CASES[name]
    fr, idx, U1, U2, g = case_inputs(name)
    P = case_weights(name)
    with torch.no_grad():
        srdf, pts, depth, rgb = O.infer(P, fr.batch, idx, fr.source_imgs_feat, fr.feature_volume,
                                        fr.match_feature, U1, U2, coarse_only=c.get("coarse_only", False))
    assert rel_err(pts, g["points"]) < EXACT
    assert rel_err(depth, g["depth"]) < EXACT < REL_TOL
    assert rel_err(rgb, g["rgb"]) < EXACT
    assert rel_err(srdf, g["srdf"]) < 1e-5


@pytest.mark.parametrize("name", ["c2_trained_like", "c2_trained_like_x64"])
def test_trained_like_statistics_match_reference_golden(name):
    """Checkpoint-like statistics (matrices x 8, LayerNorm gains up to 10, feature maps x 30 -- and x 64 / x 300; the
    modified weights travel in the fixture): dense-layer inputs ~1e3 (1e6) and an srdf head of gain ~1e3 (5e5) amplify
    op-order rounding, so the bounds are those of an fp32 evaluation of THIS network, not of the default init."""
    fr, idx, U1, U2, g = case_inputs(name)
    P = case_weights(name)
    assert float(P["ray_transformer.density_view_transformer.layers.0.norm1.weight"].max()) > 5.0
    with torch.no_grad():
        srdf, pts, depth, rgb = O.infer(P, fr.batch, idx, fr.source_imgs_feat, fr.feature_volume, fr.match_feature, U1, U2)
    e = dict(pts=rel_err(pts, g["points"]), depth=rel_err(depth, g["depth"]), rgb=rel_err(rgb, g["rgb"]),
             srdf=rel_err(srdf, g["srdf"]))
    print(f"{name}: oracle vs reference:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["pts"] < EXACT and e["depth"] < EXACT and e["rgb"] < EXACT and e["srdf"] < 1e-5


def test_rows_match_reference_golden():
    fr, idx, U1, U2, g = case_inputs("rows_small")
    P = load_weights()
    want = {}
    with torch.no_grad():
        O.infer(P, fr.batch, idx, fr.source_imgs_feat, fr.feature_volume, fr.match_feature, U1, U2, want=want)
    for tag in ("coarse", "fine"):
        w = want[tag]
        RN, SN = w["z"].shape
        assert rel_err(w["z"], g[f"{tag}.z"]) == 0.0
        assert rel_err(w["pts"], g[f"{tag}.pts"]) == 0.0
        assert rel_err(w["xy"], g[f"{tag}.xy"]) < EXACT
        assert rel_err(w["mask_z"], g[f"{tag}.mask_z"]) == 0.0
        assert rel_err(w["sim8"], g[f"{tag}.sim8"]) < EXACT
        assert rel_err(w["vol24"], g[f"{tag}.vol24"]) < EXACT
        xt = torch.from_numpy(g[f"{tag}.x_tokens"])
        assert rel_err(w["x"], xt[:, 1:]) < EXACT
        assert rel_err(w["view_out"], g[f"{tag}.view_out"]) < 1e-5
        assert rel_err(w["ray_out"], g[f"{tag}.ray_out"]) < 1e-5
        assert rel_err(w["srdf"], g[f"{tag}.srdf"]) < 1e-5
        assert rel_err(w["radiance"], g[f"{tag}.radiance"]) < 1e-5
        assert rel_err(w["weight"], g[f"{tag}.weight"]) < 1e-5
        assert rel_err(w["depth"], g[f"{tag}.depth"]) < EXACT
        assert rel_err(w["rgb"], g[f"{tag}.rgb"]) < EXACT


def test_offaxis_rows_match_reference_golden():
    """The goldens above pin the oracle on in-view rays only.  rows_offaxis.npz holds the reference's own rows (sample2rgb on
    given points) on the off-axis ray set of tests/gather_ref.py at NV = 3 and 5: samples behind source cameras, outside
    the images, outside every frustum.  Same bound as the rows above."""
    import gather_ref as G
    from helpers import load_golden
    from uforecon_amd.scene import frame_digest

    g = load_golden("rows_offaxis")
    P = load_weights()
    for NV in (3, 5):
        fr = G.frame_for(NV)
        dig = frame_digest(fr)
        assert abs(dig - float(g[f"nv{NV}.input_digest"])) <= 1e-9 * abs(dig)
        RN, SN = g[f"nv{NV}.pts"].shape[:2]
        o, d, z = G.offaxis_rays(fr, RN, SN, NV, True)
        w = G.rows(P, fr, o, d, z, torch.float32)
        assert rel_err(w["pts"], g[f"nv{NV}.pts"]) == 0.0
        s = G.geometry_shares(G.rows(P, fr, o, d, z))
        assert s["behind"] > 0.02 and s["outside_image"] > 0.2 and s["all_outside"] > 0.05, s
        assert rel_err(w["xy"], g[f"nv{NV}.xy"]) < EXACT
        assert rel_err(w["mask_z"], g[f"nv{NV}.mask_z"]) == 0.0
        assert rel_err(w["sim8"], g[f"nv{NV}.sim8"]) < EXACT
        assert rel_err(w["vol24"], g[f"nv{NV}.vol24"]) < EXACT
        assert rel_err(w["x"], g[f"nv{NV}.x"]) < EXACT


def test_train_layout_forward_matches_reference_golden():
    fr, idx, U1, U2, g = case_inputs("c5_train_fwd")
    P = load_weights()
    with torch.no_grad():
        r = O.infer(P, fr.batch, idx, fr.source_imgs_feat, fr.feature_volume, fr.match_feature, U1, U2,
                    extract_geometry=False)
    for k in ("rgb", "depth", "opacity", "weight", "rgb_2", "depth_2", "opacity_2", "weight_2", "z_val", "z_val_all"):
        assert rel_err(r[k], g[k][0]) < 1e-5, k
    assert rel_err(r["srdf"], g["srdf"][..., 0]) < 1e-5
    assert rel_err(r["srdf_2"], g["srdf_2"][..., 0]) < 1e-5
    assert rel_err(r["variance"], g["variance"]) < 1e-6
    assert rel_err(r["points_in_pixel"], g["points_in_pixel"][0]) < 1e-6 if "points_in_pixel" in r else True


@pytest.mark.parametrize("name", ["c5_train_grads", "c5_train_grads_nv4"])
def test_training_grads_match_reference_autograd(name):
    """Autograd through the oracle == autograd through the reference (loss of model.py:552-566): pins the oracle as the
    same-host checker of the HIP backward kernels."""
    from helpers import VOLUME_KEYS, golden_volume_grad, grad_rel_err

    fr, idx, U1, U2, g = case_inputs(name)
    P = {k: v.clone().requires_grad_("depthcode" not in k) for k, v in load_weights().items()}   # buffers: no grad
    for st in fr.feature_volume:
        for k in fr.feature_volume[st]:
            fr.feature_volume[st][k] = fr.feature_volume[st][k].clone().requires_grad_(True)
    r = O.infer(P, fr.batch, idx, fr.source_imgs_feat, fr.feature_volume, fr.match_feature, U1, U2,
                extract_geometry=False)
    loss = O.training_loss(r, fr.batch, idx)
    assert abs(float(loss) - float(g["loss"])) < 1e-5 * abs(float(g["loss"]))
    loss.backward()
    for k, p in P.items():
        if p.requires_grad:
            assert grad_rel_err(p.grad, g["grad." + k]) < 2e-4, k
    for key in VOLUME_KEYS:
        st, k = key.split(".")
        v = fr.feature_volume[st][k]
        assert grad_rel_err(v.grad, golden_volume_grad(g, key, v.shape)) < 2e-4, key


# ------------------------------------------------------------------ correlation-volume step
@pytest.mark.parametrize("name", ["stage1_small", "stage3_small", "nv5_stage2", "edge"])
def test_frustum_oracle_matches_reference_golden(name):
    import numpy as np
    import torch
    from oracle import frustum_oracle as FO
    from uforecon_amd.scene import correlate_digest, make_correlate_case

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"correlate_{name}.npz"))
    c = make_correlate_case(name)
    assert abs(correlate_digest(c) - float(g["input_digest"])) <= 1e-6 * abs(float(g["input_digest"]))
    sims, agg = FO.correlate(c["ref_fea"], c["src_feas"], c["ref_proj_pair"], c["src_proj_pairs"], c["depth_values"],
                             c["view_weights"])
    assert torch.equal(sims, torch.from_numpy(g["similarity"]))     # same torch ops in the same order: bit for bit
    assert torch.equal(agg, torch.from_numpy(g["aggregated"]))
