"""Host logic of HotPathTrainer's optimizer options (no GPU): argument validation, the group-to-run table handed to
cova_optim_step, the optimizer state layout and what the defaults leave exactly as before."""
import ctypes

import pytest
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, weights
from cova_web_object_detection_amd.trainer import HotPathTrainer, group_runs
from config_cases import BASE as CFG

SD = weights.seeded_state_dict(3, **{k: v for k, v in CFG.items() if k != "drop_prob"})


def trainer(**kw):
    return HotPathTrainer(CFG, SD, "cpu", **kw)


def test_optimizer_entry_points_are_exported():
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cova_optim_step", "cova_grad_norm", "cova_grad_norm_workspace_doubles"):
        assert name in _lib.parse_header() and hasattr(cdll, name), name
    # one partial per 4096 concatenated elements, at least one
    assert _lib.query("cova_grad_norm_workspace_doubles", 0) == 1
    assert _lib.query("cova_grad_norm_workspace_doubles", 4096) == 1
    assert _lib.query("cova_grad_norm_workspace_doubles", 4097) == 2
    assert _lib.query("cova_grad_norm_workspace_doubles", 9733544) == 2377


@pytest.mark.parametrize("kw, match", [
    (dict(optimizer="lamb"), "optimizer must be one of"),
    (dict(norm_type=1), "norm_type"),
    (dict(max_grad_norm=1.0, norm_type=float("inf")), "norm_type"),
    (dict(param_groups=[{"params": ("nope.",)}]), "names no parameter"),
    (dict(param_groups=[{"params": "convnet."}, {"params": ("convnet.0.weight",)}]), "claimed by param_groups"),
    (dict(param_groups=[{"params": "convnet.", "lr_scale": 0.1}]), "unknown option"),
    (dict(param_groups=[{"lr": 0.1}]), "no 'params'"),
    (dict(optimizer="sgd", nesterov=True), "Nesterov"),
    (dict(optimizer="sgd", momentum=0.9, param_groups=[{"params": "decoder.", "nesterov": True, "dampening": 0.1}]),
     "Nesterov"),
])
def test_invalid_arguments_raise(kw, match):
    with pytest.raises(ValueError, match=match):
        trainer(**kw)


def test_defaults_keep_todays_hyper_parameters_buffers_and_checkpoint():
    tr = trainer()
    assert not tr._fused and tr.optimizer == "adam" and tr.max_grad_norm is None and tr.last_grad_norm is None
    assert tr.momentum_buffer is None and tr._seg is None
    assert tr._optim_table.tensor is None and tr._run_table.tensor is None     # no device table at all
    assert {k: tr.hp[k] for k in ("lr", "weight_decay", "betas", "eps")} == dict(lr=5e-4, weight_decay=1e-3,
                                                                                  betas=(0.9, 0.999), eps=1e-8)
    n = tr.pbucket.flat.numel()
    assert tr.exp_avg.shape == (n,) and tr.exp_avg_sq.shape == (n,)
    st = tr.optimizer_state_dict()
    assert set(st) == {"step", "exp_avg", "exp_avg_sq", "hp"}
    assert st["hp"] == dict(lr=5e-4, weight_decay=1e-3, betas=(0.9, 0.999), eps=1e-8)
    # one default group of every parameter, which is the hyper-parameter dict itself
    assert len(tr.param_groups) == 1 and tr.param_groups[0] is tr.hp
    assert tr.param_groups[0]["params"] == list(tr.params)
    assert tr.optim_runs == [(0, n, 0)]


def test_group_runs_merge_adjacent_tensors_and_leave_out_frozen_ones():
    offsets = {"a": (0, 3, (3,)), "b": (4, 4, (4,)), "c": (8, 1, (1,)), "d": (12, 5, (5,)), "e": (20, 2, (2,))}
    owner = {"a": 0, "b": 0, "c": 1, "e": 1}
    assert group_runs(offsets, 24, {"d"}, owner) == [(0, 8, 0), (8, 12, 1), (20, 24, 1)]
    assert group_runs(offsets, 24, set(), dict(owner, d=1)) == [(0, 8, 0), (8, 24, 1)]


def test_param_groups_resolve_to_merged_runs_of_the_flat_bucket():
    no_decay = [k for k in SD if k.endswith(".bias") or ".bn" in k]
    no_decay = [k for k in no_decay if k in trainer().params and not k.startswith("convnet.")]
    tr = trainer(optimizer="adamw", param_groups=[{"params": ("convnet.",), "lr": 5e-5},
                                                  {"params": no_decay, "weight_decay": 0.0}],
                 frozen=("convnet.0.", "convnet.1."))
    groups = tr.param_groups
    assert len(groups) == 3 and groups[2] is tr.hp                      # the default group comes last
    assert groups[0]["lr"] == 5e-5 and groups[0]["weight_decay"] == tr.hp["weight_decay"]
    assert groups[1]["weight_decay"] == 0.0 and groups[1]["lr"] == tr.hp["lr"]
    assert all(k not in g["params"] for g in groups for k in tr.frozen)
    assert all(k.startswith("convnet.") for k in groups[0]["params"])
    assert sorted(sum((g["params"] for g in groups), [])) == sorted(k for k in tr.params if k not in tr.frozen)
    owner = {k: i for i, g in enumerate(groups) for k in g["params"]}
    flat_owner = {}
    for lo, hi, gid in tr.optim_runs:
        for k, (o, m, _) in tr.pbucket.offsets.items():
            if lo <= o < hi:
                flat_owner[k] = gid
    assert flat_owner == owner                                          # every trainable view in a run of its group
    runs = tr.optim_runs
    assert all(a[1] <= b[0] for a, b in zip(runs, runs[1:]))
    assert all(a[1] < b[0] or a[2] != b[2] for a, b in zip(runs, runs[1:]))   # adjacent runs of one group are merged
    frozen_lo = [tr.pbucket.offsets[k][0] for k in tr.frozen]
    assert not any(lo <= f < hi for f in frozen_lo for lo, hi, _ in runs)
    seg = tr._seg.tolist()                                              # device table: lo, hi, group, start
    start = 0
    for (lo, hi, gid), row in zip(runs, seg):
        assert row == [lo, hi, gid, start]
        start += hi - lo
    assert tr._optim_table.total == start and tr._seg is tr._optim_table.tensor


def test_groups_naming_only_frozen_keys_and_claiming_everything():
    tr = trainer(param_groups=[{"params": "convnet."}], frozen=("convnet.",), max_grad_norm=1.0)
    assert tr.param_groups[0]["params"] == []                           # frozen keys belong to no group
    assert tr.param_groups[1] is tr.hp and tr.optim_runs and all(g == 1 for _, _, g in tr.optim_runs)
    everything = trainer(param_groups=[{"params": list(trainer().params), "lr": 1e-2}])
    assert len(everything.param_groups) == 1 and everything.param_groups[0] is not everything.hp
    assert everything.optim_runs == [(0, everything.pbucket.flat.numel(), 0)]


def test_optimizer_state_layout_and_round_trip():
    groups = [{"params": "convnet.", "lr": 1e-4, "momentum": 0.5}]
    tr = trainer(optimizer="sgd", momentum=0.9, dampening=0.1, weight_decay=0.0, param_groups=groups)
    tr.momentum_buffer.uniform_()
    tr._buf_exists = [True, False]
    tr.step_count = 7
    tr.param_groups[0]["lr"] = 3e-4                                    # a manual schedule
    st = tr.optimizer_state_dict()
    assert st["algorithm"] == "sgd" and st["momentum_buffer_exists"] == [True, False]
    assert st["momentum_buffer"].shape == tr.pbucket.flat.shape
    assert [g["lr"] for g in st["groups"]] == [3e-4, 5e-4]
    assert st["groups"][0]["momentum"] == 0.5 and st["groups"][1]["momentum"] == 0.9
    assert st["groups"][1]["dampening"] == 0.1
    tr2 = trainer(optimizer="sgd", momentum=0.9, dampening=0.1, weight_decay=0.0, param_groups=groups)
    tr2.load_optimizer_state_dict(st)
    assert tr2.step_count == 7 and torch.equal(tr2.momentum_buffer, tr.momentum_buffer)
    assert tr2._buf_exists == [True, False] and tr2.param_groups[0]["lr"] == 3e-4


def test_an_old_adam_checkpoint_loads_and_another_algorithm_is_refused():
    old = trainer()
    old.exp_avg.fill_(0.25)
    old.step_count = 11
    old.hp["lr"] = 2e-4
    st = old.optimizer_state_dict()
    assert "algorithm" not in st
    # into a trainer that runs Adam through the fused launch (clipping, groups): moments, step and default lr
    tr = trainer(max_grad_norm=5.0, param_groups=[{"params": "decoder.", "lr": 1e-3}])
    tr.load_optimizer_state_dict(st)
    assert tr.step_count == 11 and torch.equal(tr.exp_avg, old.exp_avg) and tr.hp["lr"] == 2e-4
    assert tr.param_groups[0]["lr"] == 1e-3
    for algorithm in ("adamw", "sgd"):
        other = trainer(optimizer=algorithm)
        with pytest.raises(ValueError, match="algorithm"):
            other.load_optimizer_state_dict(st)
        with pytest.raises(ValueError, match="algorithm"):
            tr.load_optimizer_state_dict(other.optimizer_state_dict())
    with pytest.raises(ValueError, match="parameter groups"):
        trainer(param_groups=[{"params": "convnet."}]).load_optimizer_state_dict(tr.optimizer_state_dict())
