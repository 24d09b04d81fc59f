"""Host side of the optional layer2 stage (CoVA(backbone_layers=2)): state_dict keys against torchvision's layer2 naming,
the feature-map size / RoIPool scale against a CPU forward of the stack, the gradient plan's layer2 rows, and the
constructor's refusals."""
import pytest

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import engine, weights
from cova_web_object_detection_amd.models import CoVA
from cova_web_object_detection_amd.trainer import is_param_key
from layer2_oracle import dummy_forward_size
from config_cases import ADDL_SPEC as CFG

# torchvision resnet18().layer2.state_dict(): key -> shape
TV_LAYER2 = {}
for _b in (0, 1):
    for _c in ("conv1", "conv2"):
        TV_LAYER2["%d.%s.weight" % (_b, _c)] = (128, 64 if (_b, _c) == (0, "conv1") else 128, 3, 3)
        for _l in ("weight", "bias", "running_mean", "running_var"):
            TV_LAYER2["%d.bn%s.%s" % (_b, _c[-1], _l)] = (128,)
        TV_LAYER2["%d.bn%s.num_batches_tracked" % (_b, _c[-1])] = ()
TV_LAYER2["0.downsample.0.weight"] = (128, 64, 1, 1)
for _l in ("weight", "bias", "running_mean", "running_var"):
    TV_LAYER2["0.downsample.1.%s" % _l] = (128,)
TV_LAYER2["0.downsample.1.num_batches_tracked"] = ()


def test_spec_layer2_keys_and_shapes():
    spec1 = weights.state_dict_spec(**CFG)
    spec2 = weights.state_dict_spec(backbone_layers=2, **CFG)
    l2 = {k[len("convnet.5."):]: s for k, s in spec2 if k.startswith("convnet.5.")}
    assert l2 == TV_LAYER2
    # everything else as for backbone_layers=1, except the visual width (128 * 3 * 3) that the head reads
    conv1 = [(k, s) for k, s in spec1 if k.startswith("convnet.")]
    assert [(k, s) for k, s in spec2 if k.startswith("convnet.") and not k.startswith("convnet.5.")] == conv1
    assert weights.backbone_channels("resnet18", 2) == 128
    n_feat = 128 * 9 + 16 + 3
    assert dict(spec2)["gat.W_i.weight"] == (48, n_feat)
    sd = weights.seeded_state_dict(7, backbone_layers=2, **CFG)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in spec2]
    assert weights.state_dict_spec(backbone_layers=1, **CFG) == spec1


@pytest.mark.parametrize("h,w", [(64, 64), (128, 96), (97, 131), (1280, 1280), (33, 17), (200, 57)])
def test_feature_size_matches_a_dummy_forward(h, w):
    assert (engine.feature_map_size(h, 2), engine.feature_map_size(w, 2)) == dummy_forward_size(h, w)


@pytest.mark.parametrize("img_h", [64, 128, 97, 1280])
def test_module_scale_and_widths(img_h):
    m = CoVA((3, 3), img_h, 4, True, 48, 16, 0, 0.0, None, backbone_layers=2)
    assert m.roi_pool.spatial_scale == dummy_forward_size(img_h, img_h)[0] / img_h
    assert m.n_visual_feat == 128 * 9
    sd = m.state_dict()
    spec = weights.state_dict_spec(backbone_layers=2, roi_output_size=(3, 3), n_classes=4, use_context=True,
                                   hidden_dim=48, bbox_hidden_dim=16, n_additional_feat=0)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in spec]
    one = CoVA((3, 3), img_h, 4, True, 48, 16, 0, 0.0, None)
    assert not any(k.startswith("convnet.5.") for k in one.state_dict())


def test_backbone_state_dict_maps_layer2():
    import torch
    tv = {"conv1.weight": torch.randn(64, 3, 7, 7)}
    for k, s in weights.state_dict_spec(backbone_layers=2, **CFG):
        if k.startswith("convnet.1."):
            tv["bn1." + k[len("convnet.1."):]] = torch.ones(s) if s else torch.tensor(0)
        elif k.startswith(("convnet.4.", "convnet.5.")):
            tv["layer%d.%s" % (int(k[8]) - 3, k[len("convnet.4."):])] = (torch.randn(s) if s else torch.tensor(0))
    m = CoVA((3, 3), 64, 4, True, 48, 16, 0, 0.0, None, backbone_layers=2, backbone_state_dict=tv)
    assert torch.equal(m.convnet[5][0].downsample[0].weight, tv["layer2.0.downsample.0.weight"])
    assert torch.equal(m.convnet[5][1].conv2.weight, tv["layer2.1.conv2.weight"])
    del tv["layer2.1.bn2.bias"]
    with pytest.raises(RuntimeError):                       # loading stays strict
        CoVA((3, 3), 64, 4, True, 48, 16, 0, 0.0, None, backbone_layers=2, backbone_state_dict=tv)


@pytest.mark.parametrize("kw", [dict(backbone="resnet50", backbone_layers=2), dict(backbone_layers=3),
                                dict(backbone_layers=0), dict(backbone_layers=True)])
def test_constructor_refusals(kw):
    with pytest.raises(ValueError):
        CoVA((3, 3), 64, 4, True, 48, 16, 0, 0.0, None, **kw)
    with pytest.raises(ValueError):
        weights.state_dict_spec(**dict(CFG, **kw))


def keys2():
    return [k for k, _ in weights.state_dict_spec(backbone_layers=2, **CFG) if is_param_key(k)]


L1 = ["convnet.4.0.conv1.weight", "convnet.4.0.conv2.weight", "convnet.4.1.conv1.weight", "convnet.4.1.conv2.weight"]
L2 = ["convnet.5.0.conv1.weight", "convnet.5.0.conv2.weight", "convnet.5.0.downsample.0.weight",
      "convnet.5.1.conv1.weight", "convnet.5.1.conv2.weight"]
ALL2 = {"convstack", "stem", "conv1_wgrad", "bbox", "addl", "layer1"} | {"wgrad:" + k for k in L1 + L2}
HEAD = {"bbox", "addl"}


def without(ks, *prefixes):
    return [k for k in ks if not k.startswith(prefixes)]


PLAN_TABLE = [
    (keys2(), False, ALL2),                                                                   # full step
    (without(keys2(), "convnet."), False, HEAD),                                              # backbone frozen
    (without(keys2(), "convnet."), True, HEAD | {"convstack", "stem", "layer1"}),             # ... but d images
    (without(keys2(), "convnet.0.", "convnet.1.", "convnet.4."), False,                       # stem + layer1 frozen
     HEAD | {"convstack"} | {"wgrad:" + k for k in L2}),
    (without(keys2(), "convnet.0.", "convnet.1.", "convnet.4."), True,
     HEAD | {"convstack", "stem", "layer1"} | {"wgrad:" + k for k in L2}),
    (without(keys2(), "convnet.0.", "convnet.1."), False, ALL2 - {"stem", "conv1_wgrad"}),    # stem frozen
    (without(keys2(), *L2), False, ALL2 - {"wgrad:" + k for k in L2}),                        # layer2 convs frozen
    (without(keys2(), "convnet.5.1.conv2."), False, ALL2 - {"wgrad:convnet.5.1.conv2.weight"}),
    (["convnet.5.1.bn2.weight"], False, {"convstack"}),                                       # only layer2's last BN
    (["convnet.4.1.bn2.bias"], False, {"convstack", "layer1"}),                               # a layer1 BN
]


@pytest.mark.parametrize("need,want_dimg,expected", PLAN_TABLE)
def test_grad_plan_table_layer2(need, want_dimg, expected):
    assert engine.grad_plan(need, want_dimg, layer2=True) == frozenset(expected)


def test_full_plan_layer2():
    assert engine.full_plan(dict.fromkeys(keys2())) == frozenset(ALL2)
