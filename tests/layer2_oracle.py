"""CPU oracle of the optional layer2 stage (CoVA(backbone_layers=2)), composed from torch ops on top of
oracle.cova_oracle: torchvision resnet18's layer2 (two BasicBlocks 64 -> 128, block 0 at stride 2 with a 1x1 stride-2
downsample) after the oracle's conv stack.  The reference cannot express this model (models.py:49-51 keeps layer1)."""
import torch
import torch.nn.functional as F

from oracle import cova_oracle as O


def layer2(x, sd, training, routing=None):
    routing = routing or {}
    for blk in (0, 1):
        p = "convnet.5.%d." % blk
        stride = 2 if blk == 0 else 1
        idt = x
        if blk == 0:
            idt = O._bn(F.conv2d(x, sd[p + "downsample.0.weight"], None, stride=2), sd, p + "downsample.1.", training)
        y = F.conv2d(x, sd[p + "conv1.weight"], None, stride=stride, padding=1)
        y = O._relu(O._bn(y, sd, p + "bn1.", training), routing, "gate_l2_a1_%d" % blk)
        y = F.conv2d(y, sd[p + "conv2.weight"], None, stride=1, padding=1)
        y = O._bn(y, sd, p + "bn2.", training)
        x = O._relu(y + idt, routing, "gate_l2_out_%d" % blk)
    return x


def feature_map_size(img_h):
    """one more (k=3, s=2, p=1) output-size step after the oracle's stride-4 map"""
    return (O.feature_map_size(img_h) + 2 - 3) // 2 + 1


def patch(monkeypatch):
    """Make the oracle's forward (and everything built on it: loss_and_grads) the backbone_layers=2 model."""
    conv, fms = O.convnet, O.feature_map_size
    monkeypatch.setattr(O, "convnet", lambda images, sd, training, routing=None:
                        layer2(conv(images, sd, training, routing), sd, training, routing))
    monkeypatch.setattr(O, "feature_map_size", lambda h: (fms(h) + 2 - 3) // 2 + 1)


def routing(sv):
    """The ReLU gates of the HIP forward's layer2 (NHWC -> the oracle's NCHW)."""
    s = sv["conv"]["layer2"]
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu()
    return {"gate_l2_a1_0": nchw(s["a1"] > 0), "gate_l2_out_0": nchw(s["out0"] > 0),
            "gate_l2_a1_1": nchw(s["a3"] > 0), "gate_l2_out_1": nchw(s["out1"] > 0)}


def dummy_forward_size(h, w):
    """Output size of torchvision resnet18 children()[:-4] on a [1,3,h,w] page, by a CPU forward of the stack."""
    import torch.nn as nn
    layers = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
              nn.Conv2d(64, 64, 3, 1, 1, bias=False), nn.Conv2d(64, 128, 3, 2, 1, bias=False)]
    with torch.no_grad():
        return tuple(nn.Sequential(*layers).eval()(torch.zeros(1, 3, h, w)).shape[2:])
