"""Fine-tuning idioms on the GPU: per-module train/eval modes (``model.train(); model.convnet.eval()``) and frozen
parameters (``requires_grad_(False)``) through the drop-in module and HotPathTrainer.

Expected values come from the CPU oracle composed per layer: its single ``training`` flag is overridden per BatchNorm
prefix by wrapping ``cova_oracle._bn``; frozen parameters are the ones dropped from the gradient comparison.  Every
discrete decision of the oracle's backward is forced to the HIP forward's (routing), so gradients compare at the
tolerances of tests/test_model_gpu.py.  Launches are counted by entry-point name through ``_lib.PROFILE``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import engine, synthetic, weights  # noqa: E402
from cova_web_object_detection_amd.models import CoVA  # noqa: E402
from helpers import compare_grads, DEV, GRAD_TOL, LOGIT_TOL, LOSS_TOL, profiled, relerr, routing_from_saved  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
from config_cases import make_cfg  # noqa: E402

# resnet50 (2304 visual features) and RoIAlign: 2e-4, as tests/test_extension_gpu.py for these configurations (measured:
# one entry of decoder.1.bias -- analytically zero in front of a train-mode BatchNorm, i.e. rounding noise -- above 1e-4)
GRAD_TOL_EXT = 2e-4
P_DROP = 0.3


def setup(backbone="resnet18", roi_op="pool", drop_prob=0.0, seed=5):
    cfg = make_cfg((3, 3), 48, 16, drop_prob=drop_prob)
    sd = weights.seeded_state_dict(seed, logit_gain=2.0, backbone=backbone,
                                   **{k: v for k, v in cfg.items() if k != "drop_prob"})
    batch = synthetic.make_batch(2, img_h=96, boxes_per_page=[14, 9], context_size=3, seed=seed + 1)
    m = CoVA((3, 3), 96, 4, True, 48, 16, 0, drop_prob, None, backbone=backbone, roi_op=roi_op)
    m.load_state_dict(sd, strict=True)
    ocfg = dict(cfg, backbone=backbone, roi_op=roi_op)
    return ocfg, sd, batch, m.to(DEV).train()


def head_routing(sv):
    """The head's forced decisions alone (the conv stack kept no activations: nothing flows back into it)."""
    r = {}
    if sv["roi"].get("argmax") is not None:
        r["roi_argmax"] = sv["roi"]["argmax"].cpu()
    n_vis, hd = sv["n_vis"], sv["Hd"]
    r["gate_bbox"] = (sv["comb"][:, n_vis:n_vis + hd] > 0).cpu()
    r["gate_dec"] = (sv["dec"]["y"] > 0).cpu()
    for layer in sv.get("gat") or []:
        for head in layer["heads"]:
            t = torch.cat((head["t"], head["t"].new_zeros(1)))
            u = head["s"].view(-1, 1) + t[head["ctx"].clamp(min=-1)]
            r["gate_" + head["prefix"] + "leaky"] = (u > 0).cpu()
    return r


def bn_modes(m):
    return {n + ".": mod.training for n, mod in m.named_modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)}


def run_case(monkeypatch, prepare, backbone="resnet18", roi_op="pool", drop_prob=0.0, masks=None, oracle_masks=None):
    """prepare(model) sets modes / requires_grad; -> (model, saved forward state).  Checks logits, loss, every trainable
    gradient (None for the frozen ones, also after torch.optim.Adam) and every BatchNorm buffer against the oracle."""
    grad_tol = GRAD_TOL if (backbone, roi_op) == ("resnet18", "pool") else GRAD_TOL_EXT
    cfg, sd, batch, m = setup(backbone, roi_op, drop_prob)
    prepare(m)
    modes = bn_modes(m)
    if masks is not None:
        m._forced_masks = [t.to(DEV) for t in masks]
    img, bb, af, ctx = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    logits = m(img, bb, af, ctx)
    sv = logits.grad_fn.sv
    if sv["conv"] is not None and roi_op == "pool":
        routing = routing_from_saved(sv)
    elif sv["conv"] is not None:
        routing = routing_from_saved(dict(sv, roi=dict(argmax=torch.zeros(1, dtype=torch.int32))))
        routing.pop("roi_argmax")
    else:
        routing = head_routing(sv)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV))
    loss.backward()
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k not in trainable), k
    # the oracle, BatchNorm mode per prefix
    orig = O._bn
    monkeypatch.setattr(O, "_bn", lambda x, s, prefix, training, momentum=0.1, eps=1e-5:
                        orig(x, s, prefix, training and modes[prefix], momentum, eps))
    loss_ref, logits_ref, grads_ref, after, _ = O.loss_and_grads(
        sd, batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"], batch["labels"],
        cfg, oracle_masks, routing)
    assert relerr(logits.detach().cpu(), logits_ref) < LOGIT_TOL
    assert abs(loss.item() - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    compare_grads({k: p.grad for k, p in m.named_parameters() if k in trainable},
                  {k: g for k, g in grads_ref.items() if k in trainable}, rtol=grad_tol, outlier_frac=0.0)
    for k, b in m.named_buffers():
        prefix = k[:k.rindex(".") + 1]
        if not modes[prefix]:
            assert torch.equal(b.cpu(), sd[k]), k                # eval mode: bitwise untouched
        elif k.endswith("num_batches_tracked"):
            assert int(b) == int(after[k]), k
        else:
            assert relerr(b.cpu(), after[k]) < 1e-4, k
    # torch.optim.Adam leaves the frozen parameters bitwise alone (their grad is None)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3).step()
    for k, p in m.named_parameters():
        if k not in trainable:
            assert torch.equal(p.detach(), before[k]), k
    return m, sv


def freeze(m, prefix):
    for k, p in m.named_parameters():
        if k.startswith(prefix):
            p.requires_grad_(False)


def bn_eval_backbone(m):
    m.convnet.eval()


def frozen_backbone(m):
    freeze(m, "convnet.")


def classic(m):
    m.convnet.eval()
    freeze(m, "convnet.")


def stem_frozen(m):
    freeze(m, "convnet.0.")
    freeze(m, "convnet.1.")


def layer1_convs_frozen(m):
    for k, p in m.named_parameters():
        if k.startswith("convnet.4.") and ".conv" in k:
            p.requires_grad_(False)


def mixed_block(m):                  # bna in eval, bnb in train, inside each BasicBlock; the stem BatchNorm in eval
    m.convnet[1].eval()
    for blk in m.convnet[4]:
        blk.bn1.eval()


CASES = {"bn_eval_backbone": bn_eval_backbone, "frozen_backbone": frozen_backbone, "classic": classic,
         "stem_frozen": stem_frozen, "layer1_convs_frozen": layer1_convs_frozen, "mixed_block": mixed_block}


@pytest.mark.parametrize("case", list(CASES))
def test_finetune_case_matches_per_layer_oracle(monkeypatch, case):
    run_case(monkeypatch, CASES[case])


def test_classic_frozen_backbone_resnet50(monkeypatch):
    run_case(monkeypatch, classic, backbone="resnet50")


def test_classic_frozen_backbone_roialign(monkeypatch):
    run_case(monkeypatch, classic, roi_op="align")


@pytest.mark.parametrize("case", ["stem_frozen", "layer1_convs_frozen", "bn_eval_backbone"])
def test_finetune_case_resnet50(monkeypatch, case):
    run_case(monkeypatch, CASES[case], backbone="resnet50")


def test_first_dropout_in_eval_mode_is_the_identity(monkeypatch):
    """model.decoder[0].eval() alone, p > 0: its keep-mask is not applied (the oracle gets an all-keep mask), the second
    Dropout still applies its own."""
    _, _, batch, _ = setup()
    n, T = batch["bboxes"].shape[0], 576 + 16 + 48
    rs = np.random.RandomState(9)
    masks = [torch.from_numpy((rs.uniform(size=(n, T)) > P_DROP).astype(np.uint8)) for _ in range(2)]
    keep = torch.full((n, T), 1.0 - P_DROP)
    run_case(monkeypatch, lambda m: m.decoder[0].eval(), drop_prob=P_DROP, masks=masks,
             oracle_masks=[keep, masks[1].float()])


# ---------------------------------------------------------------------------------------------- work really skipped
def launches(prepare, backbone="resnet18"):
    """(forward launches, backward launches) by entry-point name of one module step."""
    _, _, batch, m = setup(backbone)
    prepare(m)
    img, bb, af, ctx = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    labels = batch["labels"].to(DEV)
    logits, fwd = profiled(lambda: m(img, bb, af, ctx))
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, labels)
    _, bwd = profiled(lambda: loss.backward())
    return fwd, bwd


def count(prof, *prefixes):
    return sum(c for n, c in prof.items() if n.startswith(prefixes))


DGRAD = ("cova_conv3x3_wino4_full", "cova_conv3x3_wino4_full_tail")


def test_frozen_backbone_skips_the_conv_stack_backward():
    _, bwd_full = launches(lambda m: None)
    assert count(bwd_full, "cova_conv3x3_wgrad4") and count(bwd_full, "cova_conv1_wgrad") and count(bwd_full, "cova_roipool_bwd")
    fwd, bwd = launches(classic)
    assert count(bwd, "cova_conv3x3_wgrad4", "cova_conv1_wgrad", "cova_roipool_bwd", "cova_roialign_bwd") == 0, bwd
    assert count(bwd, *DGRAD) == 0 and count(bwd, "cova_conv1_dgrad", "cova_bn_relu_maxpool_bwd", "cova_pool_bwd") == 0
    # the forward: inference launches of the conv stack, nothing kept for a backward
    assert not any("bits" in n for n in fwd), fwd
    assert count(fwd, "cova_conv3x3_wino4_bnact") == 1 and count(fwd, *DGRAD) == 0, fwd
    # frozen weights with train-mode BatchNorms: the conv stack runs its train-mode forward, still no backward
    _, bwd2 = launches(frozen_backbone)
    assert count(bwd2, "cova_conv3x3_wgrad4", "cova_conv1_wgrad", "cova_roipool_bwd", *DGRAD) == 0, bwd2


def test_frozen_stem_skips_conv1_and_one_data_gradient():
    _, bwd_full = launches(lambda m: None)
    _, bwd = launches(stem_frozen)
    assert count(bwd, "cova_conv1_wgrad") == 0 and count(bwd_full, "cova_conv1_wgrad") == 1
    assert count(bwd, *DGRAD) == count(bwd_full, *DGRAD) - 1, (bwd, bwd_full)
    assert count(bwd, "cova_conv3x3_wgrad4_partial") == 4


def test_frozen_layer1_convs_skip_their_weight_gradients():
    _, bwd = launches(layer1_convs_frozen)
    assert count(bwd, "cova_conv3x3_wgrad4") == 0, bwd
    assert count(bwd, "cova_conv1_wgrad") == 1
    # one frozen 3x3 weight: three partial launches and one finish over the three remaining slots
    _, bwd1 = launches(lambda m: m.convnet[4][1].conv2.weight.requires_grad_(False))
    assert count(bwd1, "cova_conv3x3_wgrad4_partial") == 3 and count(bwd1, "cova_conv3x3_wgrad4_finish") == 1


@pytest.mark.parametrize("backbone", ["resnet18", "resnet50"])
def test_agreeing_layer_modes_and_the_full_plan_issue_todays_launches(backbone):
    """A mode mapping in which every layer is in train (eval) mode and the plan of an all-trainable step issue exactly the
    launches of the single flag and of plan=None, with bit-identical results."""
    cfg, sd, batch, m = setup(backbone)
    params = {k: v.to(DEV) for k, v in sd.items() if k in O.param_keys(sd)}
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    labels = batch["labels"].to(DEV)
    all_train = {p: True for p in bn_modes(m)}
    all_train.update({k: True for k in engine.DROPOUT_KEYS})

    def step(modes, plan, save=True):
        buffers = {k: v.to(DEV) for k, v in sd.items() if k not in params}
        logits, sv = engine.model_fwd(cfg, params, buffers, *args, modes, save=save, plan=plan)
        if not save:
            return logits, {}
        _, dl, _ = engine.ce_sum(logits, labels)
        return logits, engine.model_bwd(sv, dl, params, plan=plan)

    (l_ref, g_ref), p_ref = profiled(lambda: step(True, None))
    (l_got, g_got), p_got = profiled(lambda: step(all_train, engine.full_plan(params)))
    assert p_got == p_ref
    assert torch.equal(l_got, l_ref) and sorted(g_got) == sorted(g_ref)
    for k in g_ref:
        assert torch.equal(g_got[k], g_ref[k]), k
    (e_ref, _), q_ref = profiled(lambda: step(False, None, save=False))
    (e_got, _), q_got = profiled(lambda: step({p: False for p in all_train}, None, save=False))
    assert q_got == q_ref and torch.equal(e_got, e_ref)


def test_one_frozen_wgrad_slot_matches_the_full_step():
    """A frozen 3x3 weight (empty finish slot, data gradient through the two-tensor prologue): every other gradient equals
    the full step's to fp32 round-off (the prologue form sums in another order) and the three remaining weight gradients
    bit for bit (their partial / finish arithmetic is unchanged)."""
    _, _, batch, m_full = setup()
    _, _, _, m = setup()
    m.convnet[4][1].conv2.weight.requires_grad_(False)
    m.convnet[4][0].conv1.weight.requires_grad_(False)
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    labels = batch["labels"].to(DEV)
    for mod in (m_full, m):
        torch.nn.CrossEntropyLoss(reduction="sum")(mod(*args), labels).backward()
    full = dict(m_full.named_parameters())
    gscale = max(float(p.grad.abs().max()) for p in full.values())
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None
            continue
        ref = full[k].grad
        if not k.startswith("convnet.") or k.startswith("convnet.4.1.bn2."):
            assert torch.equal(p.grad, ref), k      # upstream of the first changed launch: identical
        err = float((p.grad - ref).abs().max()) / max(float(ref.abs().max()), 0.01 * gscale)
        assert err < GRAD_TOL, (k, err)


# ---------------------------------------------------------------------------------------------- trainer
def test_trainer_frozen_backbone_follows_the_oracle(request):
    """HotPathTrainer(frozen=("convnet.",), bn_eval=("convnet.",)): 20 Adam steps against oracle.adam_reference on the
    trainable keys only; frozen weights, their Adam moments and the eval-mode buffers stay bitwise as they started, and
    two runs of the same seeds are bit-identical."""
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    cfg = make_cfg((3, 3), 48, 16)
    sd = weights.seeded_state_dict(77, logit_gain=2.0, **{k: v for k, v in cfg.items() if k != "drop_prob"})
    batches = [synthetic.make_batch(2, img_h=96, boxes_per_page=[20 + 3 * i, 11 + 2 * i], context_size=6, seed=900 + i)
               for i in range(3)]
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    request.addfinalizer(lambda: torch.set_num_threads(n_threads))
    keys = O.param_keys(sd)
    train_keys = [k for k in keys if not k.startswith("convnet.")]
    orig = O._bn
    mp = pytest.MonkeyPatch()
    request.addfinalizer(mp.undo)
    mp.setattr(O, "_bn", lambda x, s, prefix, training, momentum=0.1, eps=1e-5:
               orig(x, s, prefix, training and not prefix.startswith("convnet."), momentum, eps))
    runs = []
    for _ in range(2):
        tr = HotPathTrainer(cfg, sd, DEV, frozen=("convnet.",), bn_eval=("convnet.",))
        assert tr.plan is not None and "convstack" not in tr.plan
        losses = []
        for it in range(20):
            b = {k: v.to(DEV) for k, v in batches[it % 3].items() if torch.is_tensor(v)}
            loss, _ = tr.train_step(b)
            losses.append(float(loss))
        runs.append((losses, tr))
    (losses, tr), (losses2, tr2) = runs
    assert losses == losses2
    for a, b in ((tr.pbucket.flat, tr2.pbucket.flat), (tr.exp_avg, tr2.exp_avg), (tr.exp_avg_sq, tr2.exp_avg_sq)):
        assert torch.equal(a, b)
    # the oracle: Adam on the trainable keys only, the backbone's BatchNorms in eval mode
    ref_sd, state, curve = O.clone_state_dict(sd), None, []
    for it in range(20):
        b = batches[it % 3]
        loss_ref, _, grads, after, _ = O.loss_and_grads(ref_sd, b["images"], b["bboxes"], b["additional_feats"],
                                                        b["context_indices"], b["labels"], cfg, None)
        new_p, state = O.adam_reference([ref_sd[k] for k in train_keys], [grads[k] for k in train_keys], state)
        for k, p in zip(train_keys, new_p):
            after[k] = p
        ref_sd = after
        curve.append((losses[it], float(loss_ref)))
    a0, r0 = curve[0]
    assert abs(a0 - r0) <= LOSS_TOL * abs(r0)
    assert max(abs(a - r) / abs(r) for a, r in curve[:3]) < 2e-5
    for it, (a, r) in enumerate(curve):
        assert abs(a - r) <= 0.05 * abs(r) + 2e-3 * r0, (it, a, r)
    assert curve[-1][1] < curve[0][1]
    got = tr.state_dict()
    for k in got:
        if k.startswith("convnet."):
            assert torch.equal(got[k].cpu(), sd[k]), k                          # weights and eval-mode buffers
        elif k.endswith("num_batches_tracked"):
            assert int(got[k]) == 20, k
    for k in keys:
        if k.startswith("convnet."):
            o, n, _ = tr.pbucket.offsets[k]
            assert not tr.exp_avg[o:o + n].any() and not tr.exp_avg_sq[o:o + n].any(), k
