"""Host logic of the fine-tuning idioms (no GPU): the gradient plan, per-layer modes, the batch-size check per
BatchNorm1d, and HotPathTrainer's frozen / bn_eval bookkeeping."""
import pytest
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import engine, weights
from cova_web_object_detection_amd.trainer import HotPathTrainer, is_param_key
from config_cases import ADDL_SPEC as CFG


def keys(backbone="resnet18"):
    return [k for k, _ in weights.state_dict_spec(backbone=backbone, **CFG) if is_param_key(k)]


def without(ks, *prefixes):
    return [k for k in ks if not k.startswith(prefixes)]


L1_18 = ["convnet.4.0.conv1.weight", "convnet.4.0.conv2.weight", "convnet.4.1.conv1.weight", "convnet.4.1.conv2.weight"]
L1_50 = ["convnet.4.%d.%s.weight" % (b, c) for b in range(3) for c in ("conv1", "conv2", "conv3")]
ALL_18 = {"convstack", "stem", "conv1_wgrad", "bbox", "addl"} | {"wgrad:" + k for k in L1_18}
ALL_50 = {"convstack", "stem", "conv1_wgrad", "bbox", "addl"} | {"wgrad:" + k for k in L1_50}
HEAD = {"bbox", "addl"}

# (backbone, parameters that need a gradient, images need one?) -> expected stages
PLAN_TABLE = [
    ("resnet18", keys(), False, ALL_18),                                                            # full step
    ("resnet50", keys("resnet50"), False, ALL_50),
    ("resnet18", without(keys(), "convnet."), False, HEAD),                                         # (a) frozen backbone
    ("resnet50", without(keys("resnet50"), "convnet."), False, HEAD),
    ("resnet18", without(keys(), "convnet."), True, HEAD | {"convstack", "stem"}),                  # ... but d images
    ("resnet18", without(keys(), "convnet.0."), False, ALL_18 - {"conv1_wgrad"}),                   # (b) conv1 frozen
    ("resnet18", without(keys(), "convnet.0.", "convnet.1."), False, ALL_18 - {"conv1_wgrad", "stem"}),  # (c) stem
    ("resnet18", without(keys(), "convnet.0.", "convnet.1."), True, ALL_18 - {"conv1_wgrad"}),
    ("resnet50", without(keys("resnet50"), "convnet.0.", "convnet.1."), False, ALL_50 - {"conv1_wgrad", "stem"}),
    ("resnet18", without(keys(), *L1_18), False, ALL_18 - {"wgrad:" + k for k in L1_18}),            # (d) layer1 convs
    ("resnet18", without(keys(), "convnet.4.1.conv2."), False, ALL_18 - {"wgrad:convnet.4.1.conv2.weight"}),
    ("resnet18", without(keys(), "bbox_feat_encoder."), False, ALL_18 - {"bbox"}),                   # (e) positional encoder
    # fallbacks: work that is only partly frozen is done whole
    ("resnet18", without(keys(), "bbox_feat_encoder.0."), False, ALL_18),          # encoder Linear frozen, its BN not
    ("resnet18", without(keys(), "convnet.1."), False, ALL_18),                    # stem BN frozen, conv1 trainable
    ("resnet18", without(keys(), "convnet.4.0.bn1.", "convnet.4.1."), False, ALL_18 - {"wgrad:convnet.4.1.conv1.weight",
                                                                                       "wgrad:convnet.4.1.conv2.weight"}),
    ("resnet18", without(keys(), "decoder.", "gat."), False, ALL_18),              # a frozen head costs nothing extra
    ("resnet18", ["convnet.4.1.bn2.weight"], False, {"convstack"}),                # only the last BN: no stem, no wgrad
    ("resnet18", [], False, set()),
    ("resnet18", [], True, {"convstack", "stem"}),
]


@pytest.mark.parametrize("backbone,need,want_dimg,expected", PLAN_TABLE)
def test_grad_plan_table(backbone, need, want_dimg, expected):
    assert engine.grad_plan(need, want_dimg) == frozenset(expected)


def test_full_plan_is_every_stage():
    params = dict.fromkeys(keys())
    assert engine.full_plan(params) == frozenset(ALL_18)


def test_layer_modes():
    assert engine.is_train(True, "convnet.1.") and not engine.is_train(False, "decoder.2.")
    modes = {"convnet.1.": False, "decoder.0": False}
    assert not engine.is_train(modes, "convnet.1.") and not engine.is_train(modes, "decoder.0")
    assert engine.is_train(modes, "convnet.4.0.bn1.") and engine.is_train(modes, "decoder.3")    # unnamed: train
    assert engine.collapse_modes({"a.": True, "b.": True}) is True
    assert engine.collapse_modes({"a.": False, "b.": False}) is False
    assert engine.collapse_modes({"a.": True, "b.": False}) == {"a.": True, "b.": False}


def test_one_box_batch_raises_only_for_a_train_mode_batchnorm1d():
    """torch's _verify_batch_size fires at the first TRAIN-mode BatchNorm1d of the forward, with that layer's width."""
    cfg = dict(CFG, n_additional_feat=0)
    img, bb = torch.zeros(1, 3, 32, 32), torch.zeros(1, 5)
    af, ctx = torch.zeros(1, 0), torch.zeros(1, 4, dtype=torch.long)
    T = 64 * 9 + 16 + 48
    for modes, width in ((True, 16), ({"bbox_feat_encoder.1.": False}, T),
                         ({"bbox_feat_encoder.1.": False, "decoder.2.": False}, None),
                         ({"convnet.1.": False}, 16), (False, None)):
        if width is None:
            engine.check_batch(cfg, img, bb, af, ctx, modes)
        else:
            with pytest.raises(ValueError, match=r"torch.Size\(\[1, %d\]\)" % width):
                engine.check_batch(cfg, img, bb, af, ctx, modes)


def _trainer(**kw):
    cfg = dict(CFG, backbone="resnet18")
    sd = weights.seeded_state_dict(3, **cfg)
    return HotPathTrainer(cfg, sd, "cpu", **kw), sd


def test_trainer_defaults_are_todays_step():
    tr, _ = _trainer()
    assert tr.frozen == frozenset() and tr.modes is True and tr.plan is None and not tr.conv_frozen


def test_trainer_frozen_and_bn_eval_bookkeeping():
    tr, sd = _trainer(frozen=("convnet.",), bn_eval=("convnet.", "decoder.2.weight"))
    assert tr.frozen == {k for k in tr.params if k.startswith("convnet.")}
    assert tr.conv_frozen and "convstack" not in tr.plan and {"bbox", "addl"} <= tr.plan
    bns = [k[:-len("running_mean")] for k in sd if k.endswith("running_mean")]
    assert tr.modes == {p: False for p in bns if p.startswith("convnet.") or p == "decoder.2."}
    # Adam runs cover exactly the trainable tensors (+ the alignment padding between adjacent ones)
    covered = torch.zeros(tr.pbucket.flat.numel(), dtype=torch.bool)
    for lo, hi in tr._adam_runs:
        covered[lo:hi] = True
    for k, (o, n, _) in tr.pbucket.offsets.items():
        assert bool(covered[o:o + n].all()) == (k not in tr.frozen) and bool(covered[o:o + n].any()) == (k not in tr.frozen), k
    # the state_dict layout does not change
    ref, _ = _trainer()
    assert list(tr.state_dict()) == list(ref.state_dict())
    assert tr.pbucket.offsets == ref.pbucket.offsets


def test_trainer_frozen_head_tensor_splits_the_adam_runs():
    tr, _ = _trainer(frozen=("gat.W_j.weight", "convnet.0.weight"))
    assert len(tr._adam_runs) == 2
    assert tr.plan == engine.grad_plan([k for k in tr.params if k not in tr.frozen])
    assert "conv1_wgrad" not in tr.plan and "stem" in tr.plan and not tr.conv_frozen


def test_trainer_rejects_names_that_match_nothing():
    with pytest.raises(ValueError, match="frozen"):
        _trainer(frozen=("convnet.9.",))
    with pytest.raises(ValueError, match="bn_eval"):
        _trainer(bn_eval=("decoder.1.",))
