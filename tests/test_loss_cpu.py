"""Host logic of the configurable criterion (no GPU): the trainer's new keywords and their refusals, what the defaults
leave exactly as before, the drop-in CrossEntropyLoss module's arguments, and the declared entry points."""
import ctypes

import pytest
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, engine, weights
from cova_web_object_detection_amd.models import CrossEntropyLoss
from cova_web_object_detection_amd.trainer import HotPathTrainer, LossMetrics
from config_cases import BASE as CFG

SD = weights.seeded_state_dict(3, **{k: v for k, v in CFG.items() if k != "drop_prob"})


def trainer(**kw):
    return HotPathTrainer(CFG, SD, "cpu", **kw)


def test_loss_entry_points_are_declared_and_exported():
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.parse_header()
    for name in ("cova_ce_loss_fwd", "cova_ce_loss_bwd", "cova_ce_loss_workspace_doubles", "cova_ce_sum"):
        assert name in protos and hasattr(cdll, name), name
    # four doubles per slice of 2048 rows, at least one slice
    for n, doubles in ((0, 4), (2, 4), (2048, 4), (2049, 8), (20000, 40)):
        assert _lib.query("cova_ce_loss_workspace_doubles", n) == doubles, n


@pytest.mark.parametrize("kw, match", [
    (dict(class_weight=[1.0, 2.0, 3.0]), "class_weight must hold n_classes"),
    (dict(class_weight=[[1.0, 2.0], [3.0, 4.0]]), "class_weight must hold n_classes"),
    (dict(class_weight=[1.0, -2.0, 3.0, 1.0]), "finite and non-negative"),
    (dict(class_weight=[1.0, float("nan"), 3.0, 1.0]), "finite and non-negative"),
    (dict(class_weight=[1.0, float("inf"), 3.0, 1.0]), "finite and non-negative"),
    (dict(label_smoothing=-0.1), "label_smoothing"),
    (dict(label_smoothing=1.0), "label_smoothing"),
    (dict(focal_gamma=0.5), "focal_gamma"),
    (dict(focal_gamma=-1.0), "focal_gamma"),
    (dict(focal_gamma=2.0, label_smoothing=0.1), "cannot be combined"),
    (dict(ignore_index=0), "names a class"),
    (dict(ignore_index=3), "names a class"),
    (dict(loss_reduction="none"), "loss reduction"),
    (dict(loss_reduction="avg"), "loss reduction"),
])
def test_invalid_criterion_arguments_raise(kw, match):
    with pytest.raises(ValueError, match=match):
        trainer(**kw)


def test_default_trainer_keeps_the_ce_sum_path_and_checkpoint_formats():
    tr = trainer()
    assert tr.loss_path == "cova_ce_sum" and tr._criterion() is None
    assert tr.class_weight is None and tr.metrics is None
    assert tr.loss_options == dict(label_smoothing=0.0, focal_gamma=0.0, ignore_index=None, loss_reduction="sum")
    with_opts = trainer(class_weight=[1.0, 5.0, 5.0, 0.0], label_smoothing=0.1, ignore_index=-100, loss_reduction="mean",
                        track_metrics=True)
    assert set(with_opts.optimizer_state_dict()) == set(tr.optimizer_state_dict())
    assert list(with_opts.state_dict()) == list(tr.state_dict())


@pytest.mark.parametrize("kw", [dict(class_weight=[1.0, 2.0, 2.0, 2.0]), dict(label_smoothing=0.1), dict(focal_gamma=2.0),
                                dict(ignore_index=-100), dict(ignore_index=4), dict(loss_reduction="mean"),
                                dict(track_metrics=True)])
def test_any_option_selects_the_new_path(kw):
    tr = trainer(**kw)
    assert tr.loss_path == "cova_ce_loss"
    opts = tr._criterion()
    assert set(opts) == {"label_smoothing", "focal_gamma", "ignore_index", "reduction"}


def test_loss_options_are_read_and_checked_at_every_step():
    tr = trainer(class_weight=[1, 2, 3, 4])
    assert tr.class_weight.dtype == torch.float32 and tr.class_weight.tolist() == [1.0, 2.0, 3.0, 4.0]
    tr.loss_options["label_smoothing"] = 0.2
    assert tr._criterion()["label_smoothing"] == 0.2
    tr.loss_options["focal_gamma"] = 2.0
    with pytest.raises(ValueError, match="cannot be combined"):
        tr._criterion()
    plain = trainer()
    plain.loss_options["loss_reduction"] = "mean"          # an edit of the dict alone moves the step to the new path
    assert plain.loss_path == "cova_ce_loss"


def test_metrics_object_layout_and_reset():
    tr = trainer(track_metrics=True)
    assert isinstance(tr.metrics, LossMetrics)
    assert tr.metrics.buf.dtype == torch.int64 and tr.metrics.buf.shape == (4 * 4 + 4,)
    # host side of read(): a hand-filled buffer (confusion [[5,1],[0,2]] of a 2-class problem, sums as float64 bits)
    m = LossMetrics(2, "cpu")
    m.buf[:6] = torch.tensor([5, 1, 0, 2, 8, 3])
    m.buf[6:] = torch.tensor([12.0, 8.0], dtype=torch.float64).view(torch.int64)
    out = m.read()
    assert out["confusion"].tolist() == [[5, 1], [0, 2]] and out["kept"] == 8 and out["bad_labels"] == 3
    assert out["loss"] == 12.0 and out["loss_numerator"] == 12.0 and out["loss_denominator"] == 8.0
    assert out["recall"].tolist() == [5 / 6, 1.0] and out["precision"].tolist() == [1.0, 2 / 3]
    m.reset()
    out = m.read()
    assert not m.buf.any() and out["kept"] == 0 and all(x != x for x in out["recall"])      # NaN where undefined


@pytest.mark.parametrize("kw, match", [
    (dict(reduction="none"), "not implemented"),
    (dict(reduction="batchmean"), "loss reduction"),
    (dict(label_smoothing=1.5), "label_smoothing"),
    (dict(focal_gamma=0.3), "focal_gamma"),
    (dict(focal_gamma=2.0, label_smoothing=0.1), "cannot be combined"),
    (dict(weight=[1.0, -1.0]), "finite and non-negative"),
    (dict(weight=[[1.0, 1.0]]), "one-dimensional"),
])
def test_cross_entropy_loss_module_refuses_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        CrossEntropyLoss(**kw)


def test_cross_entropy_loss_module_mirrors_torch_and_has_no_cpu_fallback():
    ours, theirs = CrossEntropyLoss(), torch.nn.CrossEntropyLoss()
    assert (ours.ignore_index, ours.reduction, ours.label_smoothing) == (theirs.ignore_index, theirs.reduction,
                                                                         theirs.label_smoothing)
    assert ours.weight is None and ours.focal_gamma == 0.0
    w = CrossEntropyLoss(weight=[1.0, 2.0, 3.0, 4.0])
    assert "weight" in dict(w.named_buffers()) and not list(w.parameters())
    assert w.to(torch.float32).weight.tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))
    from cova_web_object_detection_amd.dropin import models as dropin_models
    assert dropin_models.CrossEntropyLoss is CrossEntropyLoss


def test_engine_option_check_normalises():
    assert engine.check_loss_options(4) == dict(label_smoothing=0.0, focal_gamma=0.0, ignore_index=None, reduction="sum")
    with pytest.raises(ValueError, match="classes"):
        engine.check_loss_options(17)
