"""`python -m uforecon_amd.similarity_field` end to end on the tests' small fixtures: a DTU scan layout
(tests/dtu_scan_golden.py) and a `--test_general` scene (tests/general_scan_golden.py).  One batch per scan, the first render
view; `sim_<scan>_<resolution>.ply`, with `--save_field` the field beside it."""
import argparse
import os

import numpy as np
import pytest
import torch

import dtu_scan_golden as G
import general_scan_golden as S
from uforecon_amd import ops
from uforecon_amd import similarity_field as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMMON = ["--test_n_view", "3", "--volume_type", "correlation", "--depth_pos_encoding", "--mvs_depth_guide", "1",
          "--explicit_similarity", "--resolution", "16", "--save_field"]


def _args():   # the smallest frame of tests/test_pipeline.py: 32x64, 3 views
    return argparse.Namespace(extract_geometry=True, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64,
                              fine_sample=64, volume_type="correlation", volume_reso=96, mvs_depth_guide=1,
                              depth_pos_encoding=True, use_dir_srdf=False, explicit_similarity=True,
                              test_coarse_only=False, test_ray_num=800, test_n_view=3, out_dir=None)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from uforecon_amd import pipeline
    from uforecon_amd.scene import fill_state_dict

    net = fill_state_dict(pipeline.UFOReconInference(_args()), 21).eval()
    path = str(tmp_path_factory.mktemp("ckpt") / "model.ckpt")
    torch.save({"state_dict": net.state_dict()}, path)
    return path


def _read_ply(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "ply" and "end_header" in lines
    V = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    F = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    body = [ln for ln in lines[lines.index("end_header") + 1:] if ln]
    assert len(body) == V + F
    verts = np.array([[float(t) for t in ln.split()[:3]] for ln in body[:V]]).reshape(-1, 3)
    faces = np.array([[int(t) for t in ln.split()[1:]] for ln in body[V:]]).reshape(-1, 3)
    assert F == 0 or (faces.min() >= 0 and faces.max() < V)
    return verts, faces


def _check_outputs(out, scan, threshold):
    """The field file is a finite (16,16,16) float32 volume; the PLY is the mesh `field_mesh` gives for it at ``threshold``."""
    assert sorted(os.listdir(out)) == ["sim_%s_16.npy" % scan, "sim_%s_16.ply" % scan]
    u = np.load(os.path.join(out, "sim_%s_16.npy" % scan))
    assert u.shape == (16, 16, 16) and u.dtype == np.float32 and np.isfinite(u).all() and np.abs(u).max() <= 1.0 + 1e-5
    verts, faces = _read_ply(os.path.join(out, "sim_%s_16.ply" % scan))
    v, f, _ = SF.field_mesh(torch.from_numpy(u).to(DEV), [-1.] * 3, [1.] * 3, level=threshold)
    assert len(verts) == len(v) and np.array_equal(faces, f.cpu().numpy().reshape(-1, 3))
    assert len(v) == 0 or np.abs(verts - v.cpu().numpy()).max() < 1e-6       # "%f" keeps six decimals
    return u, len(v)


def test_command_on_a_dtu_scan_layout(tmp_path_factory, checkpoint, tmp_path):
    root, scan = G.write_scan(tmp_path_factory.mktemp("dtu"))
    g, cfg = G.golden(), G.cases()["set0"]
    argv = ["--test_dir", root, "--load_ckpt", checkpoint, "--scans", scan[4:], "--set", "0",
            "--test_ref_view", *[str(v) for v in cfg["test_view_pair"]], "--img_wh", *[str(v) for v in cfg["img_wh"]],
            "--original_img_wh", *[str(int(v)) for v in g["original_img_wh"]], *COMMON]
    out = str(tmp_path / "first")
    assert SF.main(argv + ["--out_dir", out]) == 0
    u, _ = _check_outputs(out, scan, 0.99)
    # --threshold is honoured: at the field's median there is a surface
    out2 = str(tmp_path / "second")
    level = float(np.median(u))
    assert SF.main(argv + ["--out_dir", out2, "--threshold", repr(level), "--min_views", "0"]) == 0
    u2, n_verts = _check_outputs(out2, scan, level)
    assert np.array_equal(u, u2) and (n_verts > 0 or float(u.min()) == float(u.max()))
    assert ops.status_poll(True) == 0


def test_command_with_test_general(tmp_path_factory, checkpoint, tmp_path):
    root, scan = S.write_scene(tmp_path_factory.mktemp("general"))
    refs = S.cases()["mvimage"]["test_ref_view"]
    argv = ["--test_dir", root, "--load_ckpt", checkpoint, "--test_general", "--test_scan", scan, "--dataset", "mvimage", "--use_mask",
            "--test_ref_view", *[str(v) for v in refs], "--img_wh", "64", "32", *COMMON]
    out = str(tmp_path / "out")
    assert SF.main(argv + ["--out_dir", out, "--min_views", "1"]) == 0
    u, _ = _check_outputs(out, scan, 0.99)
    assert ops.status_poll(True) == 0

