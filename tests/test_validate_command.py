"""`python -m uforecon_amd.validate`: main.py's flag names, and one line with exit code 2 for what the mirror does not implement."""
import json
import subprocess
import sys

import pytest

from dtu_scan_golden import golden as scan_golden
from uforecon_amd import validate as V

OK = ["--root_dir", "a", "--scans", "scan3", "--depth_pos_encoding", "--explicit_similarity", "--mvs_depth_guide", "1",
      "--test_ref_view", "23", "24", "33", "--train_n_view", "4"]
MAIN_PY = ["--root_dir", "--load_ckpt", "--logdir", "--test_n_view", "--train_n_view", "--test_ref_view", "--view_selection_type",
           "--val_only", "--coarse_sample", "--fine_sample", "--volume_type", "--mvs_depth_guide", "--depth_pos_encoding",
           "--explicit_similarity", "--use_dir_srdf", "--ndepths", "--depth_inter_r", "--cr_base_chs"]


def test_help_lists_the_references_names():
    r = subprocess.run([sys.executable, "-m", "uforecon_amd.validate", "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in MAIN_PY + ["--pair_filepath", "--split_filepath", "--scans", "--seed"]:
        assert flag in r.stdout, flag


def test_flags_carry_main_py_defaults():
    ref = {f["flag"]: f for f in json.loads(str(scan_golden()["main_py_flags"]))}      # recorded from main.py's own parser calls
    ours = {a.option_strings[0]: a for a in V.make_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    for flag in MAIN_PY:
        r, a = ref[flag], ours[flag]
        if r["action"] == "store_true":
            assert a.nargs == 0 and a.default is False, flag
        else:
            assert a.default == r["default"] and a.nargs == r["nargs"] and (a.choices or None) == r["choices"], flag
    args = V.make_parser().parse_args(OK)
    assert V.unimplemented(args) is None and args.pair_filepath is None and args.logdir == "./checkpoints/random_sample"


@pytest.mark.parametrize("extra", [["--volume_type", "featuregrid"], ["--use_dir_srdf"], ["--ndepths", "64,32,8"],
                                   ["--mvs_depth_guide", "0"], ["--train_n_view", "5"], ["--train_n_view", "9", "--val_only"],
                                   ["--test_ref_view"] + [str(v) for v in range(20, 29)]])
def test_unimplemented_flag_values_exit_with_one_line(extra, capsys):
    with pytest.raises(SystemExit) as e:
        V.main(OK + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "Traceback" not in err and extra[0] in err.strip().splitlines()[-1]


def test_new_symbols_in_header_and_binding():
    """the five additive entry points: declared in include/ufr.h, bound in _lib with as many arguments, ABI number unchanged"""
    import ctypes as C
    import os
    import re

    from uforecon_amd import _lib
    from uforecon_amd.build import SOURCES

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ufr.h")).read()
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["ufr_render_rays_pair", "ufr_frame_metrics_workspace_bytes", "ufr_frame_metrics", "ufr_frame_preview_u8", "ufr_depth_gt_prepare"]
    for name in names:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        rtype, args = _lib.SIGNATURES[name]
        assert len(args) == len(m.group(2).split(",")), name
        assert rtype is (C.c_size_t if m.group(1) == "size_t" else C.c_int), name
    assert "frame_metrics.hip" in SOURCES and "api_validate.hip" in SOURCES
    for f in ("frame_metrics.hip", "api_validate.hip"):
        assert os.path.exists(os.path.join(root, "uforecon_amd", "csrc", f))
