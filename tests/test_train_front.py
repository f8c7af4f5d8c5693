"""The training front door without a GPU: optim.Adam's host form and state format, the ray draw's host form, the train
command's flags, epoch order, checkpoint bookkeeping and file, and the prefetch wrapper."""
import argparse
import ctypes as C
import json
import os
import re
import threading

import pytest
import torch

import train_front_ref as R
from dtu_scan_golden import golden as scan_golden
from uforecon_amd import _lib, ops, optim, pipeline
from uforecon_amd import train as T
from uforecon_amd.extract_geometry import load_checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
NUMELS = (1, 3, 65, 1328)
LR = 1e-3


# ------------------------------------------------------------------------------------------------------- optim.Adam
@pytest.fixture(scope="module")
def adam_ref():
    params, grads = R.adam_case(NUMELS)
    want, bounds = R.adam_bounds(params, grads, LR)
    return params, grads, want, bounds


def _within(got, want, bounds, label):
    for i, (g, w, b) in enumerate(zip(got, want, bounds)):
        err = float((g - w).abs().max())
        print(f"{label}: tensor {i} ({w.numel()} elements) error {err:.3e}, bound {b:.3e}")
        assert err <= b, (label, i, err, b)


def test_adam_host_form_follows_torch_in_float64(adam_ref):
    params, grads, want, bounds = adam_ref
    got, opt = R.run_adam(lambda ps: optim.Adam(ps, lr=LR), params, grads)
    _within(got, want, bounds, "optim.Adam on the CPU")
    assert all(float((w - p.double()).abs().max()) > 1e-4 for w, p in zip(want[:4], params[:4]))      # the steps moved them
    assert torch.equal(got[4], params[4].double())                                                    # never a gradient: untouched
    ps = opt.param_groups[0]["params"]
    assert [float(opt.state[p]["step"]) for p in ps[:4]] == [5.0, 4.0, 5.0, 5.0]                       # the skipped tensor's count
    assert ps[4] not in opt.state                                                                     # state is created at the first gradient


def test_adam_state_dict_is_torchs(adam_ref):
    params, grads, _, _ = adam_ref
    _, ours = R.run_adam(lambda ps: optim.Adam(ps, lr=LR), params, grads)
    _, theirs = R.run_adam(lambda ps: torch.optim.Adam(ps, lr=LR), params, grads)
    a, b = ours.state_dict(), theirs.state_dict()
    assert set(a) == set(b) and len(a["param_groups"]) == len(b["param_groups"]) == 1
    assert a["param_groups"][0] == b["param_groups"][0]                                                # keys AND values
    assert set(a["state"]) == set(b["state"]) == {0, 1, 2, 3}
    for i in a["state"]:
        assert set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"])
        assert a["state"][i]["step"].dtype == b["state"][i]["step"].dtype and a["state"][i]["step"].device == b["state"][i]["step"].device


@pytest.mark.parametrize("first,second", [("ours", "torch"), ("torch", "ours")])
def test_adam_state_moves_between_the_classes(adam_ref, first, second):
    params, grads, want, bounds = adam_ref
    make = {"ours": lambda ps: optim.Adam(ps, lr=LR), "torch": lambda ps: torch.optim.Adam(ps, lr=LR)}
    got, opt = R.run_adam(make[first], params, grads, make_second=make[second], switch_at=3)
    _within(got, want, bounds, f"{first} for 3 steps, its state loaded into {second} for 2")
    assert [float(opt.state[p]["step"]) for p in opt.param_groups[0]["params"][:4]] == [5.0, 4.0, 5.0, 5.0]


def test_adam_refuses_what_it_does_not_implement():
    p = torch.zeros(3, requires_grad=True)
    opt = optim.Adam([p], lr=LR)
    opt.param_groups[0]["amsgrad"] = True
    p.grad = torch.ones(3)
    with pytest.raises(ops.UfrError, match="amsgrad"):
        opt.step()


def test_adam_step_advances_the_version_counters():
    p = torch.zeros(3, requires_grad=True)
    opt = optim.Adam([p], lr=LR)
    p.grad = torch.ones(3)
    v = p._version
    opt.step()
    assert p._version > v


# ---------------------------------------------------------------------------------------------------- ops.select_rays
def test_select_rays_host_form_is_the_stable_argsort():
    u = R.quantised_uniforms(5000)
    s = torch.sort(u).values
    k_tie = next(j for j in range(1000, 5000) if s[j - 1] == s[j])         # the k-th and the (k+1)-th smallest are equal
    for k in (1, 7, k_tie, 1024, 5000):
        assert torch.equal(ops.select_rays(u, k), torch.sort(u, stable=True).indices[:k])
    same = torch.full((300,), 0.25)
    assert torch.equal(ops.select_rays(same, 64), torch.arange(64))
    with pytest.raises(ops.UfrError):
        ops.select_rays(u, 5001)
    with pytest.raises(ops.UfrError):
        ops.select_rays(u.double(), 3)


def test_entry_points_header_binding_and_argument_errors():
    from uforecon_amd.build import SOURCES, build_library

    text = open(os.path.join(os.path.dirname(HERE), "include", "ufr.h")).read()
    assert "#define UFR_ABI_VERSION 507" in text and _lib.ABI_VERSION == 507
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ufr_adam_table_capacity", "ufr_adam_step", "ufr_select_rays_workspace_bytes", "ufr_select_rays"):
        m = re.search(r"\b(int|size_t|int32_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        rtype, args = _lib.SIGNATURES[name]
        assert len(args) == (0 if m.group(2).strip() == "void" else len(m.group(2).split(","))), name
    assert "train_step.hip" in SOURCES and "api_train.hip" in SOURCES
    assert C.sizeof(_lib.AdamTensor) == 56
    if not os.path.exists(_lib.LIB_PATH):
        build_library(verbose=False)
    lib = _lib.load()
    assert lib.ufr_adam_table_capacity() == 64
    assert lib.ufr_select_rays_workspace_bytes(5000, 4097) == 0 and b"k=4097" in lib.ufr_last_error()
    assert lib.ufr_select_rays_workspace_bytes(2 ** 24 + 1, 8) == 0
    assert lib.ufr_select_rays_workspace_bytes(7, 8) == 0
    assert lib.ufr_select_rays_workspace_bytes(2 ** 24, 4096) > 0
    assert lib.ufr_select_rays(None, 5000, 4097, None, None, 0, None) == -1 and b"k=4097" in lib.ufr_last_error()
    assert lib.ufr_select_rays(None, 5000, 16, None, None, 0, None) == -1 and b"null" in lib.ufr_last_error()
    t = (_lib.AdamTensor * 1)()
    t[0].numel = 4
    assert lib.ufr_adam_step(t, 1, 1e-3, 0.9, 0.999, 1e-8, None) == -1 and b"null pointer" in lib.ufr_last_error()
    assert lib.ufr_adam_step(None, 0, 1e-3, 0.9, 0.999, 1e-8, None) == 0                      # nothing to do


# ------------------------------------------------------------------------------------------------------- the command
OK = ["--root_dir", "a", "--scans", "scan3", "--depth_pos_encoding", "--explicit_similarity", "--mvs_depth_guide", "1",
      "--test_ref_view", "23", "24", "33", "--train_n_view", "4", "--batch_size", "1"]
MAIN_PY = ["--root_dir", "--max_epochs", "--batch_size", "--uforecon_lr", "--load_ckpt", "--train_ray_num", "--coarse_sample",
           "--fine_sample", "--weight_rgb", "--weight_depth", "--logdir", "--test_n_view", "--train_n_view", "--test_ref_view",
           "--view_selection_type", "--mvs_depth_guide", "--volume_type", "--volume_reso", "--depth_pos_encoding",
           "--explicit_similarity", "--use_dir_srdf", "--val_only", "--ndepths", "--depth_inter_r", "--cr_base_chs"]


def test_flags_carry_main_py_defaults():
    ref = {f["flag"]: f for f in json.loads(str(scan_golden()["main_py_flags"]))}      # recorded from main.py's own parser calls
    ours = {a.option_strings[0]: a for a in T.make_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    for flag in MAIN_PY:
        r, a = ref[flag], ours[flag]
        if r["action"] == "store_true":
            assert a.nargs == 0 and a.default is False, flag
        else:
            assert a.default == r["default"] and a.nargs == r["nargs"] and (a.choices or None) == r["choices"], flag
    for flag in ("--split_filepath", "--val_split_filepath", "--scans", "--pair_filepath", "--seed", "--precision", "--max_steps",
                 "--max_val_frames", "--train_items", "--log_every", "--resume", "--prefetch"):
        assert flag in ours, flag
    args = T.make_parser().parse_args(OK)
    assert T.unimplemented(args) is None and args.uforecon_lr == 1e-4 and args.max_epochs == 16


@pytest.mark.parametrize("extra", [["--batch_size", "2"], ["--volume_type", "featuregrid"], ["--mvs_depth_guide", "0"],
                                   ["--train_n_view", "5"], ["--test_ref_view"] + [str(v) for v in range(20, 29)],
                                   ["--train_ray_num", "4097"], ["--val_only"], ["--use_dir_srdf"]])
def test_unimplemented_flag_values_exit_with_one_line(extra, capsys):
    with pytest.raises(SystemExit) as e:
        T.main(OK + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "Traceback" not in err and extra[0] in err.strip().splitlines()[-1]


def test_default_batch_size_is_main_pys_and_refused(capsys):
    with pytest.raises(SystemExit) as e:
        T.main(OK[:-2])
    assert e.value.code == 2 and "--batch_size 2" in capsys.readouterr().err


def test_epoch_permutation_depends_on_seed_and_epoch_alone():
    items = [7, 275, 3, 12, 99, 41, 0, 8]
    a = T.epoch_permutation(3, 0, items)
    assert sorted(a) == sorted(items) and a == T.epoch_permutation(3, 0, tuple(items))
    torch.manual_seed(123)                       # the process-wide generator has no say
    assert a == T.epoch_permutation(3, 0, items)
    assert a != T.epoch_permutation(3, 1, items) and a != T.epoch_permutation(4, 0, items)
    assert T.step_seed(3, 5) == T.step_seed(3, 5) != T.step_seed(3, 6)


def test_top_k_keeps_the_best_files(tmp_path):
    keeper = T.TopK(2)
    kept_after = []
    for epoch, score in enumerate([0.5, 0.3, 0.4, 0.6, 0.3]):
        path = str(tmp_path / ("epoch=%02d.ckpt" % epoch))
        if keeper.wants(score):
            open(path, "w").write("x")
            keeper.add(path, score)
        kept_after.append(sorted(os.listdir(tmp_path)))
    assert kept_after == [["epoch=00.ckpt"], ["epoch=00.ckpt", "epoch=01.ckpt"], ["epoch=01.ckpt", "epoch=02.ckpt"],
                          ["epoch=01.ckpt", "epoch=02.ckpt"], ["epoch=01.ckpt", "epoch=04.ckpt"]]
    assert not keeper.wants(0.3) and keeper.wants(0.29)       # mode='min': an equal score does not replace a kept file


def _train_args():
    return argparse.Namespace(extract_geometry=False, test_sample_coarse=64, test_sample_fine=64, coarse_sample=64, fine_sample=64,
                              volume_type="correlation", volume_reso=96, mvs_depth_guide=1, depth_pos_encoding=True,
                              use_dir_srdf=False, explicit_similarity=True, test_coarse_only=False, train_ray_num=1024,
                              test_n_view=3, train_n_view=4, logdir=None, uforecon_lr=1e-4, weight_rgb=1.0, weight_depth=1.0)


def test_checkpoint_of_a_cpu_model_has_the_reference_keys_and_reloads_strict(tmp_path):
    ref = json.load(open(os.path.join(HERE, "golden", "reference_state_dict_shapes.json")))
    net = pipeline.UFOReconTraining(_train_args(), tune_convolutions=False)
    opt = net.configure_optimizers()
    frozen = [p for n, p in net.named_parameters() if "transmvsnet" in n]
    assert frozen and not any(p.requires_grad for p in frozen)
    group = opt.param_groups[0]["params"]
    assert opt.param_groups[0]["lr"] == 1e-4 and any(p is net.pre_conv.weight for p in group)
    assert len(group) + len(frozen) == len(list(net.parameters())) and not any(any(p is q for q in frozen) for p in group)
    net.train()
    assert net.training and net.feature_volume.training and net.ray_transformer.training
    assert not any(m.training for m in net.transmvsnet.modules())           # the frozen encoder stays on its running statistics
    # one host-form step on the ray path's parameters, so that the file holds an optimizer state
    for p in net.ray_transformer.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    path = str(tmp_path / "checkpoints" / "epoch=00.ckpt")
    T.save_checkpoint(path, net, opt, epoch=0, global_step=1, score=0.25)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) >= {"state_dict", "epoch", "global_step", "optimizer_states", "monitor"}
    assert set(ck["state_dict"]) == set(ref) and len(ref) == 530
    assert ck["epoch"] == 0 and ck["global_step"] == 1 and ck["monitor"] == {"val/loss_depth_fine": 0.25}
    other = pipeline.UFOReconInference(_train_args(), tune_convolutions=False)
    load_checkpoint(other, path)                                             # strict
    sd = net.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    again = torch.optim.Adam([p for n, p in other.named_parameters() if "transmvsnet" not in n], lr=1e-4)
    again.load_state_dict(ck["optimizer_states"][0])                         # torch.optim.Adam's format
    assert len(again.state) == len(list(net.ray_transformer.parameters()))


# ------------------------------------------------------------------------------------------------------- Prefetch
class _FakeDataset:
    def __init__(self, fail_at=None):
        self.fail_at, self.load_threads, self.finish_threads = fail_at, [], []

    def load(self, i):
        self.load_threads.append(threading.current_thread())
        if i == self.fail_at:
            raise FileNotFoundError(2, "missing", f"item{i}.png")
        return ("decoded", i)

    def finish(self, i, loaded):
        self.finish_threads.append(threading.current_thread())
        return {"item": i, "loaded": loaded}

    def __getitem__(self, i):
        return self.finish(i, self.load(i))


@pytest.mark.parametrize("ahead", [0, 1, 3, 9])
def test_prefetch_yields_the_same_items_in_the_same_order(ahead):
    order = [5, 2, 9, 2, 0, 7, 1]
    ds = _FakeDataset()
    got = list(T.Prefetch(ds, order, ahead))
    plain = _FakeDataset()
    assert got == [(i, plain[i]) for i in order]
    main = threading.current_thread()
    assert all(t is main for t in ds.finish_threads)
    assert all((t is main) == (ahead == 0) for t in ds.load_threads)
    assert len({t for t in ds.load_threads}) <= 4


def test_prefetch_raises_a_workers_exception_at_the_consuming_index():
    order = [4, 1, 3, 6, 8]
    seen = []
    with pytest.raises(FileNotFoundError) as e:
        for i, item in T.Prefetch(_FakeDataset(fail_at=3), order, 4):
            seen.append(i)
    assert seen == [4, 1] and e.value.filename == "item3.png"
