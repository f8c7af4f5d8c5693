"""`python -m uforecon_amd.validate` end to end on the synthetic training tree of tests/dtu_train_golden.py: loader -> encoder ->
both passes -> scores -> files -> the epoch line, one 512x640 frame."""
import json

import numpy as np
import pytest

import dtu_train_golden as G
from uforecon_amd import validate as V

pytestmark = pytest.mark.gpu


def test_one_frame_of_the_test_split(tmp_path, capsys):
    root = G.write_tree(tmp_path)
    logdir = tmp_path / "log"
    rc = V.main(["--root_dir", root, "--split_filepath", str(tmp_path / "dtu_training" / "scans.txt"), "--logdir", str(logdir),
                 "--test_ref_view", "23", "24", "33", "--train_n_view", "4", "--view_selection_type", "best", "--depth_pos_encoding",
                 "--explicit_similarity", "--mvs_depth_guide", "1", "--max_frames", "1", "--seed", "3"])
    assert rc == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("scan3_light3_refview23 psnr ")                   # one line per frame, then the means
    end = json.loads(lines[-1])
    assert end == json.load(open(logdir / "val_metrics.json")) and end["frames"] == 1
    assert set(end) == {"psnr/coarse", "psnr/fine", "val/rgb_coarse", "val/rgb_fine", "val/loss_depth_coarse", "val/loss_depth_fine",
                        "loss", "frames"}
    assert all(np.isfinite(v) for v in end.values()) and end["loss"] == end["val/rgb_coarse"] + end["val/rgb_fine"]
    assert end["val/loss_depth_fine"] > 0 and 0 < end["val/rgb_fine"] < 1
    d = np.load(logdir / "depth" / "scan3" / "refview23.npy", allow_pickle=True).item()
    assert d["depth"].shape == (512, 640) and np.isfinite(d["depth"]).all() and d["extrinsic"].shape == (4, 4)
    assert (logdir / "scan3" / "depth" / "refview23.png").exists() and (logdir / "rgb" / "scan3" / "refview23.jpg").exists()
