"""The whole model on the GPU away from the one corner of the reference's hyper-parameter space the other model tests
sit in (roi_output_size (3, 3), a GAT, even head widths, K >= 4): other RoI sizes (`--roi`, main.py:60), the
`--context_size 0` ablation (main.py:58-59: no GAT, D = 0, T = F), `-cs 1` (K = 2) and head widths at which no row or
column block of the [N, T] feature matrix is 16-byte aligned.

The four configurations that have a fixture captured from the reference (tests/golden/cova_roi1_bare, cova_cs0,
cova_roi2x3_cs1, cova_roi5_odd) run through tests/test_model_gpu.py::test_full_model_matches_reference_fixture.  Here:
  * configurations held to the CPU oracle alone (the oracle is pinned to the reference at these RoI sizes and widths by
    tests/test_oracle_cpu.py), train and eval mode, with the method of tests/test_layer2_gpu.py::module_case: the HIP
    forward's discrete decisions forced into the oracle, logits at LOGIT_TOL, every gradient at GRAD_TOL of its tensor's
    scale with no outliers, running statistics at 1e-4;
  * RoIAlign at (2, 3) and (5, 5) against the oracle's roi_align, bounds of
    tests/test_extension_gpu.py::test_model_with_roialign_matches_self_oracle;
  * use_context=False ignores hidden_dim (the reference's own CoVA(use_context=False, hidden_dim=384) cannot run its
    forward; main.py always passes 0 there);
  * the reference-style train loop, HotPathTrainer and the engine step with dropout on cova_cs0 and cova_roi5_odd, with
    the bounds of tests/test_model_gpu.py::test_reference_style_train_loop_matches_fused_trainer_and_oracle and
    ::test_fused_loss_and_engine_step_match_oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import engine, synthetic, weights  # noqa: E402
from cova_web_object_detection_amd.models import CoVA  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (assert_routing_near_ties, compare_grads, DEV, GRAD_TOL,  # noqa: E402
                     load_case, LOGIT_TOL, LOSS_TOL, relerr, routing_from_saved)
from oracle import cova_oracle as O  # noqa: E402
from config_cases import make_cfg, ORACLE_CASES  # noqa: E402
from trainer_cases import seeded  # noqa: E402

KEYS = ("images", "bboxes", "additional_feats", "context_indices")


def build(cfg, img_h, sd, **kw):
    m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"],
             cfg["bbox_hidden_dim"], cfg["n_additional_feat"], cfg["drop_prob"], None, **kw)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(DEV)




def oracle_case(roi, img_h, boxes, cs, hidden, bbox_hidden, seed, train, roi_op="pool", logit_tol=LOGIT_TOL,
                grad_tol=GRAD_TOL):
    cfg = make_cfg(roi, hidden, bbox_hidden)
    sd = seeded(cfg, seed)
    batch = synthetic.make_batch(len(boxes), img_h=img_h, boxes_per_page=boxes, context_size=cs, seed=seed)
    m = build(cfg, img_h, sd, roi_op=roi_op)
    m.train(train)
    logits = m(*[batch[k].to(DEV) for k in KEYS])
    sv = logits.grad_fn.sv
    assert (sv["n_vis"], sv["T"]) == (64 * roi[0] * roi[1], 64 * roi[0] * roi[1] + bbox_hidden + hidden)
    if roi_op == "align":
        routing = routing_from_saved(dict(sv, roi=dict(argmax=torch.zeros(1, dtype=torch.int32))))
        routing.pop("roi_argmax")
    else:
        routing = routing_from_saved(sv)
    torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV)).backward()
    loss_ref, logits_ref, grads_ref, after, inter = O.loss_and_grads(
        sd, batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"], batch["labels"],
        dict(cfg, roi_op=roi_op), None, routing, training=train)
    err = relerr(logits.detach().cpu(), logits_ref)
    worst = compare_grads({k: p.grad for k, p in m.named_parameters()}, grads_ref, rtol=grad_tol, outlier_frac=0.0)
    print("roi %s %s %s: logits %.2e of the logit scale, worst gradient %s %.2e of its scale"
          % (roi, roi_op, "train" if train else "eval", err, worst[0], worst[1]))
    assert err < logit_tol, err
    if roi_op == "pool":
        assert_routing_near_ties(routing, inter, batch["bboxes"], roi, m.roi_pool.spatial_scale)
    for k, b in m.named_buffers():
        if not train:
            assert torch.equal(b.cpu(), sd[k]), k
        elif not k.endswith("num_batches_tracked"):
            assert relerr(b.cpu(), after[k]) < 1e-4, k
        else:
            assert int(b) == 1


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_other_roi_sizes_match_the_oracle(case, train):
    oracle_case(*ORACLE_CASES[case], train=train)


@pytest.mark.parametrize("roi,seed", [((2, 3), 214), ((5, 5), 215)])
def test_roialign_at_other_roi_sizes_matches_the_oracle(roi, seed):
    oracle_case(roi, 96, [15, 22], 6, 64, 16, seed, train=True, roi_op="align", logit_tol=2e-4, grad_tol=2e-4)


def test_no_context_model_ignores_hidden_dim():
    """CoVA(..., use_context=False, hidden_dim=384) is the hidden_dim=0 model: same state_dict, same bits."""
    cfg0 = make_cfg((3, 3), 0, 32, use_context=False)
    sd = seeded(cfg0, 216)
    batch = synthetic.make_batch(2, img_h=64, boxes_per_page=[12, 7], context_size=0, seed=216)
    args = [batch[k].to(DEV) for k in KEYS]
    assert tuple(args[3].shape) == (19, 0)
    runs = []
    for hidden in (0, 384):
        m = build(dict(cfg0, hidden_dim=hidden), 64, sd)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == \
            [(k, tuple(s)) for k, s in weights.state_dict_spec(**{k: v for k, v in cfg0.items() if k != "drop_prob"})]
        assert m.n_total_feat == m.n_feat == 608 and not hasattr(m, "gat")
        m.train()
        logits = m(*args)
        assert logits.grad_fn.sv["D"] == 0 and logits.grad_fn.sv["T"] == 608
        torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV)).backward()
        runs.append((logits.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert list(runs[0][1]) == list(runs[1][1])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    ref = O.forward(O.clone_state_dict(sd), batch["images"], batch["bboxes"], batch["additional_feats"],
                    batch["context_indices"], cfg0, True, None)
    assert relerr(runs[0][0].cpu(), ref) < LOGIT_TOL


# ------------------------------------------------------------------------------ trainer on the new fixture configurations
def train_loop_run(name):
    """The reference-style loop on the module, three HotPathTrainer steps -> (module losses, trainer losses, trainer)."""
    fx, cfg, sd, batch = load_case(name)
    img_h = int(fx["meta/img_h"])
    args = [batch[k].to(DEV) for k in KEYS]
    labels = batch["labels"].to(DEV)
    m = build(cfg, img_h, sd)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=5e-4, weight_decay=1e-3)          # main.py:133-135
    crit = torch.nn.CrossEntropyLoss(reduction="sum")
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = crit(m(*args), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    tr = HotPathTrainer(cfg, sd, DEV)
    dbatch = dict(zip(KEYS, args), labels=labels)
    tlosses = [tr.train_step(dbatch)[0].item() for _ in range(3)]
    return losses, tlosses, tr, m, dbatch, (fx, cfg, sd, batch)


@pytest.mark.parametrize("name", ["cova_cs0", "cova_roi5_odd"])
def test_train_loop_and_fused_trainer_on_the_new_configurations(name):
    losses, tlosses, tr, m, dbatch, (fx, cfg, sd, batch) = train_loop_run(name)
    for a, b in zip(losses, tlosses):
        assert abs(a - b) <= 1e-3 * abs(a), (losses, tlosses)
    tsd = tr.state_dict()
    # parameters within steps * lr (Adam turns a ~0 gradient into a +-lr step of arbitrary sign): the bound of
    # test_reference_style_train_loop_matches_fused_trainer_and_oracle
    bad = {k: float((v.detach() - tsd[k]).abs().max()) for k, v in m.named_parameters()
           if float((v.detach() - tsd[k]).abs().max()) > 2 * 3 * 5e-4 + 1e-3 * float(v.detach().abs().max())}
    assert not bad, bad
    assert all(torch.isfinite(v).all() for v in tsd.values())
    loss_ref, _, _, _, _ = O.loss_and_grads(sd, batch["images"], batch["bboxes"], batch["additional_feats"],
                                            batch["context_indices"], batch["labels"], cfg, None)
    assert abs(losses[0] - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    assert abs(tlosses[0] - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    assert abs(losses[0] - float(fx["train/loss"])) <= LOSS_TOL * abs(float(fx["train/loss"]))
    # state_dict(): the reference's keys, strictly loadable into the module and into a fresh trainer, same predictions
    assert sorted(tsd) == sorted(str(k) for k in fx["meta/state_keys"])
    m2 = build(cfg, int(fx["meta/img_h"]), tsd).eval()
    tr2 = HotPathTrainer(cfg, sd, DEV)
    tr2.load_state_dict(tsd)
    for k, v in tr2.state_dict().items():
        assert torch.equal(v, tsd[k]), k
    logits, pred = tr.predict(dbatch)
    assert logits.shape == (batch["bboxes"].shape[0], 4) and torch.equal(pred, logits.argmax(1))
    assert torch.equal(tr2.predict(dbatch)[0], logits)
    with torch.no_grad():
        assert relerr(m2(*[dbatch[k] for k in KEYS]).cpu(), logits.cpu()) < LOGIT_TOL
    if not cfg["use_context"]:
        for bucket in (tr.pbucket, tr.gbucket):
            assert not [k for k in bucket.offsets if k.startswith("gat.")]
            assert not [k for k in bucket.views if k.startswith("gat.")]
        assert not [k for k in tsd if k.startswith("gat.")]
        assert tr._head_offset() == tr.gbucket.split_at("bbox_feat_encoder.0.weight")
    # the whole thing again: bit-equal losses
    losses2, tlosses2 = train_loop_run(name)[:2]
    assert losses == losses2 and tlosses == tlosses2


def test_engine_step_with_dropout_at_unaligned_widths_matches_oracle():
    """engine.model_fwd + ce_sum + model_bwd with drop_prob 0.2 and injected keep-masks on the cova_roi5_odd
    configuration (T = 1710, column blocks at 1600, 1607, 1610), as test_fused_loss_and_engine_step_match_oracle does."""
    fx, cfg, sd, batch = load_case("cova_roi5_odd")
    cfg = dict(cfg, drop_prob=0.2)
    N, T = batch["bboxes"].shape[0], 1600 + 7 + 3 + 100
    rs = np.random.RandomState(3)
    masks = [torch.from_numpy((rs.uniform(size=(N, T)) > 0.2).astype(np.uint8)) for _ in range(2)]
    params = {k: v.to(DEV) for k, v in sd.items() if k in O.param_keys(sd)}
    buffers = {k: v.to(DEV) for k, v in sd.items() if k not in params}
    images, bboxes, addl, ctx = [batch[k].to(DEV) for k in KEYS]
    logits, sv = engine.model_fwd(cfg, params, buffers, images, bboxes, addl, ctx, True, masks=[m.to(DEV) for m in masks])
    assert sv["T"] == T
    loss, dl, pred = engine.ce_sum(logits, batch["labels"].to(DEV))
    routing = routing_from_saved(sv)
    grads = engine.model_bwd(sv, dl, params)
    loss_ref, logits_ref, grads_ref, after, inter = O.loss_and_grads(
        sd, batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"],
        batch["labels"], cfg, [m.float() for m in masks], routing)
    assert_routing_near_ties(routing, inter, batch["bboxes"], (5, 5), 0.25)
    assert relerr(logits.cpu(), logits_ref) < LOGIT_TOL
    assert abs(loss.item() - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    worst = compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0)
    print("cova_roi5_odd with dropout: worst gradient %s %.2e of its scale" % worst)
    for k in buffers:
        if not k.endswith("num_batches_tracked"):
            assert relerr(buffers[k].cpu(), after[k]) < 1e-4, k
