"""The optional layer2 stage on the GPU (CoVA(backbone_layers=2)).

Kernel level: every entry point of csrc/conv_nhwc.hip (forward, data gradient, weight gradient of the 3x3 s2 64->128,
3x3 s1 128->128 and 1x1 s2 64->128 convolutions) against float64 torch on the CPU, with an error no larger than that of
a plain f32 multiply-add loop over the same operands, and bit-reproducible (every launch path of the contract, bit for
bit on integer probes: tests/test_nhwc_paths_gpu.py).  Module level (square pages, a non-square page with an odd layer1
map, a one-page batch): logits and every parameter
gradient against the oracle composed in tests/layer2_oracle.py, with the HIP forward's discrete decisions forced into
the oracle's backward as in tests/test_model_gpu.py.  Trainer and fine-tuning: Adam trajectory, reruns, launch counts."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, synthetic, weights  # noqa: E402
from cova_web_object_detection_amd.models import CoVA  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import compare_grads, DEV, GRAD_TOL, profiled, routing_from_saved  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
import layer2_oracle as L2O  # noqa: E402
from config_cases import make_cfg, TRAINER_CFG  # noqa: E402

call, query = _lib.call, _lib.query
L2_LOGIT_TOL = 1e-4                                     # this suite's own bound on the logits
SHAPES = [(3, 64, 2, 1), (3, 128, 1, 1), (1, 64, 2, 0)]          # (k, Ci, stride, pad); Co = 128


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def loop_f32(a, b):
    """plain f32 FMA loop: out[m, n] = sum_k a[m, k] * b[k, n], one fused multiply-add (one rounding) per step (the
    product of two floats is exact in float64)"""
    acc = torch.zeros(a.shape[0], b.shape[1])
    a, b = a.double(), b.double()
    for k in range(a.shape[1]):
        acc = (acc.double() + a[:, k:k + 1] * b[k:k + 1]).float()
    return acc


def dgrad_loop_f32(dy, w, H, W, s, p):
    """the data gradient as ONE f32 FMA chain per input pixel over all (output channel, tap) terms: a stride-1
    convolution of the zero-stuffed, padded output gradient with the flipped, transposed weight (zeros add exactly)"""
    B, co, Ho, Wo = dy.shape
    ci, k = w.shape[1], w.shape[2]
    z = torch.zeros(B, co, (Ho - 1) * s + 1, (Wo - 1) * s + 1)
    z[:, :, ::s, ::s] = dy
    e = k - 1 - p
    z = F.pad(z, (e, e + (W + 2 * p - k) % s, e, e + (H + 2 * p - k) % s))
    wt = w.flip(2, 3).transpose(0, 1).reshape(ci, -1)
    a = F.unfold(z, k).transpose(1, 2).reshape(B * H * W, -1)
    return loop_f32(a, wt.t()).reshape(B, H, W, ci).permute(0, 3, 1, 2)


def rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def prep(w):
    co, ci, k, _ = w.shape
    wf, wd = torch.empty(k * k * ci, co, device=DEV), torch.empty(k * k * co, ci, device=DEV)
    call("cova_conv_nhwc_prep", w.to(DEV), wf, wd, co, ci, k)
    return wf, wd


@pytest.mark.parametrize("B,H,W", [(1, 9, 13), (3, 16, 16), (2, 21, 7)])
@pytest.mark.parametrize("k,ci,s,p", SHAPES)
def test_conv_nhwc_against_float64(B, H, W, k, ci, s, p):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + k + ci)
    co = 128
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * 0.05
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(B, co, Ho, Wo, generator=g)
    wf, wd = prep(w)
    cols = F.unfold(x, k, padding=p, stride=s)                          # [B, ci*k*k, L]
    M = B * Ho * Wo
    a = cols.transpose(1, 2).reshape(M, ci * k * k)
    dym = dy.permute(0, 2, 3, 1).reshape(M, co)
    runs = []
    for _ in range(2):
        out = torch.full((B, Ho, Wo, co), float("nan"), device=DEV)
        call("cova_conv_nhwc_fwd", nhwc(x), wf, out, B, H, W, ci, co, k, s, p)
        dx = torch.full((B, H, W, ci), float("nan"), device=DEV)
        call("cova_conv_nhwc_dgrad", nhwc(dy), wd, None, None, None, dx, B, H, W, ci, co, k, s, p)
        dw = torch.full((co, ci, k, k), float("nan"), device=DEV)
        ws = torch.empty(query("cova_conv_nhwc_wgrad_workspace_floats", B, Ho, Wo, ci, co, k), device=DEV)
        call("cova_conv_nhwc_wgrad", nhwc(x), nhwc(dy), dw, ws, B, H, W, ci, co, k, s, p)
        torch.cuda.synchronize()
        runs.append((out.cpu(), dx.cpu(), dw.cpu()))
    for r0, r1 in zip(*runs):
        assert torch.equal(r0, r1), "not bit-reproducible"
    out, dx, dw = runs[0]
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    ref_f = F.conv2d(x64, w64, stride=s, padding=p)
    ref_d = torch.nn.grad.conv2d_input(x.shape, w64, dy64, stride=s, padding=p)
    ref_w = torch.nn.grad.conv2d_weight(x64, w.shape, dy64, stride=s, padding=p)
    # the plain f32 loops over the same operands
    lf = loop_f32(a, w.reshape(co, -1).t()).reshape(B, Ho, Wo, co).permute(0, 3, 1, 2)
    ld = dgrad_loop_f32(dy, w, H, W, s, p)
    lw = loop_f32(dym.t().contiguous(), a).reshape(co, ci, k, k)
    pairs = [(nchw(out), lf, ref_f), (nchw(dx), ld, ref_d), (dw, lw, ref_w)]
    errs = [(rel(h, r), rel(l, r)) for h, l, r in pairs]
    errs_rms = [(rms(h, r), rms(l, r)) for h, l, r in pairs]
    print("conv_nhwc k%d s%d ci%d (hip, f32 loop) max: fwd %.2e %.2e dgrad %.2e %.2e wgrad %.2e %.2e | rms: fwd %.2e %.2e "
          "dgrad %.2e %.2e wgrad %.2e %.2e" % ((k, s, ci) + errs[0] + errs[1] + errs[2] + errs_rms[0] + errs_rms[1]
                                               + errs_rms[2]))
    # the same error class as the loop: its typical error (rms) and, with the summation-order noise of a maximum over
    # a few hundred outputs, its worst one (the factor of test_conv3x3_winograd_f4x4_split_error_class)
    for hip, loop in errs_rms:
        assert hip <= loop * 1.15, errs_rms
    for hip, loop in errs:
        assert hip <= loop * 1.5 + 1e-8, errs
    assert max(e[0] for e in errs) < 2e-6


@pytest.mark.parametrize("B,H,W", [(1, 9, 13), (2, 16, 16), (3, 11, 6)])
def test_stride2_dgrad_joins_the_downsample(B, H, W):
    """the 3x3 s2 and the 1x1 s2 data gradients land on one map in ONE launch; a 1x1-only call writes zeros at the
    positions it does not reach; an addend is added"""
    g = torch.Generator().manual_seed(B + H + W)
    w3, w1 = torch.randn(128, 64, 3, 3, generator=g) * 0.05, torch.randn(128, 64, 1, 1, generator=g) * 0.1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy3, dy1 = torch.randn(B, 128, Ho, Wo, generator=g), torch.randn(B, 128, Ho, Wo, generator=g)
    add = torch.randn(B, 64, H, W, generator=g)
    _, wd3 = prep(w3)
    _, wd1 = prep(w1)
    dx = torch.full((B, H, W, 64), float("nan"), device=DEV)
    call("cova_conv_nhwc_dgrad", nhwc(dy3), wd3, nhwc(dy1), wd1, nhwc(add), dx, B, H, W, 64, 128, 3, 2, 1)
    only1 = torch.full((B, H, W, 64), float("nan"), device=DEV)
    call("cova_conv_nhwc_dgrad", nhwc(dy1), wd1, None, None, None, only1, B, H, W, 64, 128, 1, 2, 0)
    ref3 = torch.nn.grad.conv2d_input((B, 64, H, W), w3.double(), dy3.double(), stride=2, padding=1)
    ref1 = torch.nn.grad.conv2d_input((B, 64, H, W), w1.double(), dy1.double(), stride=2)
    ref = ref3 + ref1 + add.double()
    assert rel(nchw(dx), ref) < 2e-6
    o1 = nchw(only1)
    assert rel(o1, ref1) < 2e-6
    assert torch.equal(o1[:, :, 1::2], torch.zeros_like(o1[:, :, 1::2]))
    assert torch.equal(o1[:, :, :, 1::2], torch.zeros_like(o1[:, :, :, 1::2]))


# ----------------------------------------------------------------------------------------------------- module level
def setup(img_h=64, roi_op="pool", seed=11, boxes=(13, 7), img_w=None):
    cfg = make_cfg((3, 3), 48, 16)
    sd = weights.seeded_state_dict(seed, logit_gain=2.0, backbone_layers=2,
                                   **{k: v for k, v in cfg.items() if k != "drop_prob"})
    batch = synthetic.make_batch(len(boxes), img_h=img_h, img_w=img_w, boxes_per_page=list(boxes), context_size=3,
                                 seed=seed + 1)
    m = CoVA((3, 3), img_h, 4, True, 48, 16, 0, 0.0, None, roi_op=roi_op, backbone_layers=2)
    m.load_state_dict(sd, strict=True)
    return dict(cfg, roi_op=roi_op), sd, batch, m.to(DEV)


def full_routing(sv, align):
    if align:
        r = routing_from_saved(dict(sv, roi=dict(argmax=torch.zeros(1, dtype=torch.int32))))
        r.pop("roi_argmax")
    else:
        r = routing_from_saved(sv)
    r.update(L2O.routing(sv))
    return r


def module_case(monkeypatch, img_h, roi_op="pool", train=True, prepare=None, want_dimg=False, img_w=None, boxes=(13, 7)):
    L2O.patch(monkeypatch)
    cfg, sd, batch, m = setup(img_h, roi_op, boxes=boxes, img_w=img_w)
    m.train(train)
    if prepare is not None:
        prepare(m)
    modes = {n + ".": mod.training for n, mod in m.named_modules()
             if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)}
    img, bb, af, ctx = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    if want_dimg:
        img.requires_grad_(True)
    logits = m(img, bb, af, ctx)
    sv = logits.grad_fn.sv
    routing = full_routing(sv, roi_op == "align")
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV))
    loss.backward()
    orig = O._bn
    monkeypatch.setattr(O, "_bn", lambda x, s, prefix, training, momentum=0.1, eps=1e-5:
                        orig(x, s, prefix, training and modes[prefix], momentum, eps))
    images = batch["images"].clone().requires_grad_(want_dimg)
    loss_ref, logits_ref, grads_ref, after, _ = O.loss_and_grads(
        sd, images, batch["bboxes"], batch["additional_feats"], batch["context_indices"], batch["labels"], cfg, None,
        routing, training=train)
    assert rel(logits.detach().cpu(), logits_ref.double()) < L2_LOGIT_TOL
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k not in trainable), k
    compare_grads({k: p.grad for k, p in m.named_parameters() if k in trainable},
                  {k: g for k, g in grads_ref.items() if k in trainable}, rtol=GRAD_TOL, outlier_frac=0.0)
    for k, b in m.named_buffers():
        prefix = k[:k.rindex(".") + 1]
        if not (train and modes[prefix]):
            assert torch.equal(b.cpu(), sd[k]), k
        elif not k.endswith("num_batches_tracked"):
            assert rel(b.cpu(), after[k].double()) < 1e-4, k
    if want_dimg:
        assert rel(img.grad.cpu(), images.grad.double()) < 1e-4
    return m, batch, sd


@pytest.mark.parametrize("img_h", [64, 128])
@pytest.mark.parametrize("train", [True, False])
def test_module_matches_composed_oracle(monkeypatch, img_h, train):
    module_case(monkeypatch, img_h, train=train)


@pytest.mark.parametrize("train", [True, False])
def test_module_non_square_page_with_an_odd_layer1_map(monkeypatch, train):
    """100 x 132 pixels: layer1's map is 25 x 33, odd on both sides (the four parity classes of the stride-2 data gradient
    differ in size), layer2's 13 x 17"""
    assert L2O.dummy_forward_size(100, 132) == (13, 17)
    m, batch, _ = module_case(monkeypatch, 100, train=train, img_w=132)
    assert batch["images"].shape == (2, 3, 100, 132)


@pytest.mark.parametrize("train", [True, False])
def test_module_one_page_batch(monkeypatch, train):
    m, batch, _ = module_case(monkeypatch, 64, train=train, boxes=(17,))
    assert batch["images"].shape[0] == 1


def test_module_images_grad(monkeypatch):
    module_case(monkeypatch, 64, want_dimg=True)


def test_module_roialign(monkeypatch):
    module_case(monkeypatch, 128, roi_op="align")


def test_module_layer2_eval_and_frozen_stem(monkeypatch):
    """model.convnet[5].eval(): layer2's running statistics untouched; stem + layer1 frozen: None gradients"""
    def prep(m):
        m.convnet[5].eval()
        for k, p in m.named_parameters():
            if k.startswith(("convnet.0.", "convnet.1.", "convnet.4.")):
                p.requires_grad_(False)
    module_case(monkeypatch, 64, prepare=prep)


def test_module_state_dict_round_trip_and_no_grad(monkeypatch):
    L2O.patch(monkeypatch)
    cfg, sd, batch, m = setup(64)
    m2 = CoVA((3, 3), 64, 4, True, 48, 16, 0, 0.0, None, backbone_layers=2)
    m2.load_state_dict(m.state_dict(), strict=True)
    m2.to(DEV).eval()
    m.eval()
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    with torch.no_grad():
        a, b = m(*args), m2(*args)
    assert torch.equal(a, b)
    ref = O.forward(O.clone_state_dict(sd), batch["images"], batch["bboxes"], batch["additional_feats"],
                    batch["context_indices"], cfg, False)
    assert rel(a.cpu(), ref.double()) < L2_LOGIT_TOL
    vis = m._get_visual_features(args[0], args[1])
    assert vis.shape == (args[1].shape[0], 128 * 9)


def test_multihead_gat(monkeypatch):
    L2O.patch(monkeypatch)
    batch = synthetic.make_batch(2, img_h=64, boxes_per_page=[9, 6], context_size=3, seed=4)
    m = CoVA((3, 3), 64, 4, True, 48, 16, 0, 0.0, None, n_heads=2, n_gat_layers=2, backbone_layers=2).to(DEV)
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    logits = m(*args)
    torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV)).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ----------------------------------------------------------------------------------------------------- trainer
TCFG = dict(TRAINER_CFG, backbone_layers=2)


def trainer_run(steps=3, frozen=()):
    sd = weights.seeded_state_dict(3, logit_gain=2.0, **{k: v for k, v in TCFG.items() if k != "drop_prob"})
    tr = HotPathTrainer(TCFG, sd, DEV, frozen=frozen)
    batches = [synthetic.make_batch(2, img_h=64, boxes_per_page=[11, 8], context_size=3, seed=20 + i, device=DEV)
               for i in range(steps)]
    grads = []
    for b in batches:
        tr.forward_backward(b)
        grads.append({k: v.clone() for k, v in tr.grads.items()})
        tr.optimizer_step()
    torch.cuda.synchronize()
    return tr, sd, batches, grads


def test_trainer_adam_trajectory_and_reruns():
    tr, sd, batches, grads = trainer_run()
    tr2, *_ = trainer_run()
    assert torch.equal(tr.pbucket.flat, tr2.pbucket.flat), "two runs differ"
    assert all(k in tr.state_dict() for k in sd)
    # the CPU Adam on the HIP gradients follows the same trajectory
    keys = list(tr.params)
    ps, state = [sd[k].float() for k in keys], None
    for g in grads:
        ps, state = O.adam_reference(ps, [g[k].cpu() for k in keys], state)
    for k, p in zip(keys, ps):
        assert rel(tr.params[k].cpu(), p.double()) < 1e-5, k
    page_start = torch.tensor([0, 11, 19], dtype=torch.int64, device=DEV)
    topk, correct = tr.evaluate(batches[0], page_start, k=1)
    assert topk.shape == (2, 4, 1)


def test_finetune_stem_and_layer1_frozen_launches():
    cfg, sd, batch, m = setup(64)
    m.train()
    for k, p in m.named_parameters():
        if k.startswith(("convnet.0.", "convnet.1.", "convnet.4.")):
            p.requires_grad_(False)
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    logits = m(*args)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV))
    _, bwd = profiled(lambda: loss.backward())
    assert bwd.get("cova_conv_nhwc_wgrad") == 5
    assert bwd.get("cova_conv_nhwc_dgrad") == 3                   # the three stride-1 ones; not block 0's stride-2 one
    assert not [n for n in bwd if n.startswith(("cova_conv1", "cova_conv3x3", "cova_pool_bwd", "cova_bn_relu_maxpool"))]
    for k, p in m.named_parameters():
        assert (p.grad is None) == k.startswith(("convnet.0.", "convnet.1.", "convnet.4.")), k
    # full step: the stride-2 data gradient and layer1's backward are issued
    cfg, sd, batch, m = setup(64)
    logits = m.train()(*args)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV))
    _, bwd = profiled(lambda: loss.backward())
    assert bwd.get("cova_conv_nhwc_dgrad") == 4
    assert bwd.get("cova_conv1_wgrad_poolbwd", 0) + bwd.get("cova_conv1_wgrad", 0) == 1


def test_trainer_frozen_layer1():
    tr, sd, batches, grads = trainer_run(steps=2, frozen=("convnet.0.", "convnet.1.", "convnet.4."))
    assert "layer1" not in tr.plan and "wgrad:convnet.5.0.conv1.weight" in tr.plan
    for k in tr.params:
        if k.startswith(("convnet.0.", "convnet.1.", "convnet.4.")):
            assert torch.equal(tr.params[k].cpu(), sd[k]), k
