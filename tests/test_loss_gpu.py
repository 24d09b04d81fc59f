"""The configurable criterion on the GPU: cova_ce_loss_fwd / cova_ce_loss_bwd through the C ABI against cova_ce_sum (bit
anchor) and against torch on the CPU in float64 (semantics; tests/loss_oracle.py), the device metrics, HotPathTrainer with
criterion options end to end (launches, no host synchronisation, trajectories against the oracle, two ranks against the
single-process step) and the drop-in CrossEntropyLoss module."""
import math
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import cova_amd  # noqa: E402,F401  (spawned workers re-import this module without conftest.py)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from cova_web_object_detection_amd import engine, synthetic, weights  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, CrossEntropyLoss  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer, shard_batch  # noqa: E402
import loss_oracle as LO  # noqa: E402
import syncbn_cases as SB  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
from config_cases import TRAINER_CFG as CFG  # noqa: E402
from helpers import close, DEV, free_port, LOSS_TOL, profiled  # noqa: E402
from trainer_cases import dev_batch, no_decay, trainer_setup  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_GATE = 1e-5        # tests/test_kernels_gpu.py's gate of cova_ce_sum's loss (relative)
GRAD_GATE = 1e-5        # close(): max error over max reference
NEW = ("cova_ce_loss_fwd", "cova_ce_loss_bwd")


def make(n, nc, seed, ignore=None):
    """logits randn * 4, labels 97 % class 0, about 8 % of the rows ignored when an ignore label is given"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, nc, generator=g) * 4
    labels = torch.where(torch.rand(n, generator=g) < 0.97, torch.zeros(n, dtype=torch.int64),
                         torch.randint(1, nc, (n,), generator=g))
    if ignore is not None:
        labels[torch.rand(n, generator=g) < 0.08] = ignore
    return logits, labels


def class_weights(nc, seed=5):
    w = torch.rand(nc, generator=torch.Generator().manual_seed(seed)) * 4 + 0.5
    w[1] = 0.0
    return w


def run(logits, labels, weight=None, label_smoothing=0.0, focal_gamma=0.0, ignore_index=None, reduction="sum",
        metrics=None, grad_scale=None):
    """fwd + bwd on device copies -> (acc, pred, loss, dlogits)"""
    opts = dict(label_smoothing=label_smoothing, focal_gamma=focal_gamma, ignore_index=ignore_index, reduction=reduction)
    lg, lb = logits.to(DEV), labels.to(DEV)
    w = None if weight is None else weight.to(DEV)
    acc, pred = engine.ce_loss_fwd(lg, lb, w, opts, metrics)
    loss, dl = engine.ce_loss_bwd(lg, lb, w, opts, acc, grad_scale=grad_scale)
    return acc, pred, loss, dl


def one_ulp(a, b):
    a, b = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    return bool(a == b) or bool(torch.nextafter(a, b) == b)


def modes(nc):
    """the issue's grid: {no weights, weights with one zero} x {eps 0, 0.1} x {no ignore, ignore} x {sum, mean}, plus the
    focal loss at gamma 1, 2, 3.5 with and without weights"""
    out = []
    for w in (None, class_weights(nc)):
        for eps in (0.0, 0.1):
            for ig in (None, -100):
                for red in ("sum", "mean"):
                    out.append(dict(weight=w, label_smoothing=eps, ignore_index=ig, reduction=red))
        for gamma in (1.0, 2.0, 3.5):
            out.append(dict(weight=w, focal_gamma=gamma, ignore_index=-100, reduction="mean" if gamma == 2.0 else "sum"))
    return out


def describe(kw):
    return ", ".join("%s=%s" % (k, "given" if k == "weight" and v is not None else v) for k, v in kw.items())


# ------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", [2, 311, 1440, 20000])
def test_defaults_reproduce_ce_sum(n):
    logits, labels = make(n, 4, 100 + n)
    loss_ref, dl_ref, pred_ref = engine.ce_sum(logits.to(DEV), labels.to(DEV))
    acc, pred, loss, dl = run(logits, labels)
    assert torch.equal(dl, dl_ref) and torch.equal(pred, pred_ref)
    print("N %d: loss %r, cova_ce_sum %r" % (n, loss.item(), loss_ref.item()))
    assert one_ulp(loss.item(), loss_ref.item())
    assert acc[2].item() == n and acc[1].item() == n


@pytest.mark.parametrize("nc", [2, 4, 7])
def test_loss_and_dlogits_against_float64(nc):
    n = 1440
    for i, kw in enumerate(modes(nc)):
        logits, labels = make(n, nc, 7 * nc + i, kw.get("ignore_index"))
        loss_ref, dl_ref = LO.loss_and_dlogits(logits, labels, **kw)
        acc, pred, loss, dl = run(logits, labels, **kw)
        err = abs(loss.item() - float(loss_ref)) / abs(float(loss_ref))
        gerr = float((dl.cpu().double() - dl_ref).abs().max() / dl_ref.abs().max())
        print("NC %d  %-70s loss err %.2e  dlogits err %.2e" % (nc, describe(kw), err, gerr))
        assert err <= LOSS_GATE, (describe(kw), err)
        close(dl, dl_ref, GRAD_GATE, describe(kw))
        assert torch.equal(pred.cpu(), logits.argmax(1))
        kept = labels != -100 if kw.get("ignore_index") is not None else torch.ones(n, dtype=torch.bool)
        assert acc[2].item() == int(kept.sum())
        assert not dl.cpu()[~kept].any()


def test_saturated_and_all_ignored_batches_stay_finite():
    nc, n = 4, 256
    logits = torch.randn(n, nc, generator=torch.Generator().manual_seed(3))
    hot = torch.arange(n) % nc
    logits[torch.arange(n), hot] += 100.0
    labels = hot.clone()
    labels[n // 2:] = (hot[n // 2:] + 1) % nc            # the second half is wrongly labelled
    for kw in modes(nc):
        kw = dict(kw, ignore_index=None)
        acc, pred, loss, dl = run(logits, labels, **kw)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(acc).all()), \
            describe(kw)
        assert torch.equal(pred.cpu(), hot)
    for kw in (dict(), dict(weight=class_weights(nc), label_smoothing=0.1), dict(focal_gamma=2.0)):
        acc, pred, loss, dl = run(logits, torch.full((n,), -100), ignore_index=-100, reduction="mean", **kw)
        assert loss.item() == 0.0 and not dl.any() and acc.tolist() == [0.0, 0.0, 0.0]
        assert torch.equal(pred.cpu(), hot)


def test_out_of_range_labels_are_skipped_and_counted():
    nc, n = 4, 3000
    logits, labels = make(n, nc, 11)
    bad = torch.zeros(n, dtype=torch.bool)
    bad[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:40]] = True
    dirty = labels.clone()
    dirty[bad] = torch.tensor([-100, nc, 2 ** 40, -1]).repeat(10)
    w = class_weights(nc)
    for kw in (dict(), dict(weight=w), dict(weight=w, label_smoothing=0.1, reduction="mean"), dict(focal_gamma=2.0)):
        metrics = torch.zeros(nc * nc + 4, dtype=torch.int64, device=DEV)
        acc, pred, loss, dl = run(logits, dirty, metrics=metrics, **kw)
        acc_c, _, loss_c, dl_c = run(logits[~bad], labels[~bad], **kw)
        assert metrics[nc * nc + 1].item() == 40 and metrics[nc * nc].item() == n - 40 == acc[2].item()
        assert int(metrics[:nc * nc].sum()) == n - 40
        assert torch.equal(pred.cpu(), logits.argmax(1))
        assert not dl.cpu()[bad].any()
        # the float64 sums run over other slices of rows (N differs): equal to rounding of the float64 fold
        assert torch.allclose(acc, acc_c, rtol=1e-12, atol=0.0)
        if kw.get("reduction", "sum") == "sum":
            assert torch.equal(dl.cpu()[~bad], dl_c.cpu())       # per-row values: the very bits
        else:
            close(dl.cpu()[~bad], dl_c, 1e-6, "mean: 1/denominator may round the other way")
        assert abs(loss.item() - loss_c.item()) <= 2.0 ** -22 * abs(loss_c.item())


def test_two_runs_are_bit_equal_and_metrics_accumulate():
    nc = 4
    w = class_weights(nc)
    kw = dict(weight=w, label_smoothing=0.1, ignore_index=-100, reduction="mean")
    logits, labels = make(20000, nc, 21, -100)
    a, b = run(logits, labels, **kw), run(logits, labels, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    metrics = torch.zeros(nc * nc + 4, dtype=torch.int64, device=DEV)
    conf = np.zeros((nc, nc), dtype=np.int64)
    kept = bad = 0
    num = den = den_cpu = 0.0
    for i, n in enumerate((1440, 20000, 311)):
        logits, labels = make(n, nc, 30 + i, -100)
        labels[5], labels[7] = nc, -1
        acc, pred, _, _ = run(logits, labels, metrics=metrics, **kw)
        pred = pred.cpu()
        ok = (labels >= 0) & (labels < nc)
        np.add.at(conf, (labels[ok].numpy(), pred[ok].numpy()), 1)
        kept, bad = kept + int(ok.sum()), bad + 2
        num, den = num + acc[0].item(), den + acc[1].item()
        den_cpu += float(w.double()[labels[ok]].sum())
    got = metrics.cpu()
    assert got[:nc * nc].view(nc, nc).numpy().tolist() == conf.tolist()
    assert got[nc * nc].item() == kept and got[nc * nc + 1].item() == bad
    sums = got[nc * nc + 2:].view(torch.float64).tolist()
    assert abs(sums[0] - num) <= 1e-12 * abs(num) and abs(sums[1] - den) <= 1e-12 * den
    assert abs(sums[1] - den_cpu) <= 1e-12 * den_cpu


def test_too_many_classes_are_refused():
    logits, labels = make(8, 17, 1)
    with pytest.raises(engine._lib.CovaHipError, match="10001"):
        run(logits, labels)


# ------------------------------------------------------------------------------------------------- trainer
def test_default_step_launches_ce_sum_and_options_launch_the_new_pair():
    sd, batches = trainer_setup()
    tr = HotPathTrainer(CFG, sd, DEV)
    prof = profiled(lambda: tr.forward_backward(dev_batch(batches[0])))[1]
    assert prof.get("cova_ce_sum") == 1 and not any(n in prof for n in NEW), prof
    tr = HotPathTrainer(CFG, sd, DEV, class_weight=[1.0, 4.0, 4.0, 4.0])
    prof = profiled(lambda: tr.forward_backward(dev_batch(batches[0])))[1]
    assert [prof.get(n) for n in NEW] == [1, 1] and "cova_ce_sum" not in prof, prof


def test_train_step_with_options_makes_no_host_synchronisation():
    sd, batches = trainer_setup()
    tr = HotPathTrainer(CFG, sd, DEV, class_weight=[1.0, 4.0, 4.0, 4.0], loss_reduction="mean", track_metrics=True,
                        max_grad_norm=0.5)
    bs = [dev_batch(b) for b in batches]
    tr.train_step(bs[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in bs[1:]:
            loss, pred = tr.train_step(b)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    out = tr.metrics.read()
    n = sum(b["labels"].numel() for b in batches)
    assert out["kept"] == n == int(out["confusion"].sum()) and out["bad_labels"] == 0
    assert loss.is_cuda and math.isfinite(out["loss"]) and out["loss"] > 0
    tr.metrics.reset()
    assert tr.metrics.read()["kept"] == 0


def with_ignored(batches):
    out = []
    for b in batches:
        b = dict(b, labels=b["labels"].clone())
        b["labels"][3::7] = -100
        out.append(b)
    return out


# Learning rates: the gates below can only be asked of a trajectory that its own reference determines to that accuracy.
# Measured on the CPU with reference_curve alone: against a copy whose initial parameters are moved by one f32 rounding
# (1.2e-7 relative), the focal reference at lr 5e-4 (loss 48 -> 33 -> 71 -> 11: it overshoots) differs from itself by 1e-3
# from step 4 on and by 1e-1 at step 10 (ReLU / pooling decisions flip), at lr 5e-5 by at most 1.2e-6 at every step
# while still falling 48 -> 3.9.  "mean" divides the gradient by ~200 but Adam's step does not depend on that scale:
# its reference at lr 5e-4 falls 1.79 -> 0.66.
TRAJECTORIES = {
    "ce_weights_smoothing_ignore_mean_adam": dict(
        crit=dict(weight=[1.0, 3.0, 2.0, 4.0], label_smoothing=0.1, ignore_index=-100, reduction="mean"),
        optimizer="adam", lr=5e-4, clip=False),
    "focal_weights_sum_adamw_clipped": dict(
        crit=dict(weight=[1.0, 3.0, 2.0, 4.0], focal_gamma=2.0, reduction="sum"),
        optimizer="adamw", lr=5e-5, clip=True),
}


def trainer_kw(crit):
    return dict(class_weight=crit.get("weight"), label_smoothing=crit.get("label_smoothing", 0.0),
                focal_gamma=crit.get("focal_gamma", 0.0), ignore_index=crit.get("ignore_index"),
                loss_reduction=crit.get("reduction", "sum"))


def reference_curve(case, sd, batches, max_norm=None):
    """14 steps of the oracle with the criterion swapped, clip_grad_norm_ and torch.optim (setup of
    test_trainer_adamw_groups_and_clipping_follow_the_oracle) -> (losses, max_norm)"""
    keys = O.param_keys(sd)
    lr, wd = case["lr"], 1e-2
    ref_sd = O.clone_state_dict(sd)
    ps = {k: ref_sd[k].clone().requires_grad_(True) for k in keys}
    if case["optimizer"] == "adamw":
        nd = [k for k in keys if no_decay(k)]
        opt = torch.optim.AdamW([dict(params=[ps[k] for k in nd], weight_decay=0.0),
                                 dict(params=[ps[k] for k in keys if k not in nd])], lr=lr, weight_decay=wd)
    else:
        opt = torch.optim.Adam(list(ps.values()), lr=lr, weight_decay=wd)
    curve = []
    for it in range(14):
        loss_ref, _, grads, after = LO.loss_and_grads(ref_sd, batches[it % 3], CFG, **case["crit"])
        if it == 0 and case["clip"]:
            max_norm = 0.5 * math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
        for k in keys:
            ps[k].grad = grads[k].clone().view_as(ps[k])
        if case["clip"]:
            torch.nn.utils.clip_grad_norm_(list(ps.values()), max_norm)
        opt.step()
        for k in keys:
            after[k] = ps[k].detach().clone()
        ref_sd = after
        curve.append(float(loss_ref))
    return curve, max_norm


@pytest.mark.parametrize("name", sorted(TRAJECTORIES))
def test_trainer_with_criterion_options_follows_the_oracle(request, name):
    case = TRAJECTORIES[name]
    sd, batches = trainer_setup()
    if case["crit"].get("ignore_index") is not None:
        batches = with_ignored(batches)
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    request.addfinalizer(lambda: torch.set_num_threads(n_threads))
    ref, max_norm = reference_curve(case, sd, batches)
    kw = dict(lr=case["lr"], weight_decay=1e-2, optimizer=case["optimizer"], **trainer_kw(case["crit"]))
    if case["optimizer"] == "adamw":
        kw["param_groups"] = [{"params": [k for k in O.param_keys(sd) if no_decay(k)], "weight_decay": 0.0}]
    if case["clip"]:
        kw["max_grad_norm"] = max_norm
    tr = HotPathTrainer(CFG, sd, DEV, **kw)
    got = [float(tr.train_step(dev_batch(batches[it % 3]))[0]) for it in range(14)]
    for it, (a, r) in enumerate(zip(got, ref)):
        print("%s step %2d: loss %.6f  oracle %.6f  rel %.2e" % (name, it, a, r, abs(a - r) / abs(r)))
    r0 = ref[0]
    assert abs(got[0] - r0) <= LOSS_TOL * abs(r0)
    assert max(abs(a - r) / abs(r) for a, r in zip(got[:3], ref[:3])) < 2e-5
    for it, (a, r) in enumerate(zip(got, ref)):
        assert abs(a - r) <= 0.05 * abs(r) + 2e-3 * r0, (it, a, r)
    assert ref[-1] < ref[0]


def test_validation_loss_is_the_criterion_on_the_eval_forward():
    sd, batches = trainer_setup()
    crit = dict(weight=[1.0, 3.0, 2.0, 4.0], label_smoothing=0.1, ignore_index=-100, reduction="mean")
    b = with_ignored(batches)[0]
    for c in (crit, dict(weight=[1.0, 3.0, 2.0, 4.0], focal_gamma=2.0), dict()):
        tr = HotPathTrainer(CFG, sd, DEV, **trainer_kw(c))
        bb = dev_batch(b if c.get("ignore_index") is not None else batches[0])
        loss = tr.loss(bb)
        assert loss.dim() == 0 and loss.is_cuda
        logits, _ = tr.predict(bb)
        ref = LO.criterion(logits.cpu().double(), bb["labels"].cpu(), **c)
        assert abs(loss.item() - float(ref)) <= 1e-5 * abs(float(ref)), (c, loss.item(), float(ref))


# ------------------------------------------------------------------------------------------------- two ranks
DDP_KW = dict(class_weight=[1.0, 3.0, 0.5, 4.0], ignore_index=-100, loss_reduction="mean", track_metrics=True)


def ddp_batch(case):
    """tests/test_syncbn_gpu.py's batch (pages of 21, 34 | 9, 40 boxes: rank 0 gets 55 boxes, rank 1 49) with ignored
    boxes: "uneven" = every 5th box of rank 0's pages and every 3rd of rank 1's; "one_empty" = all of rank 1's."""
    b = SB.batch()
    labels = b["labels"].clone()
    labels[0:55:5] = -100
    if case == "uneven":
        labels[55::3] = -100
    else:
        labels[55:] = -100
    return dict(b, labels=labels)


def _ddp_worker(rank, world, port, out_dir, case):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg, wcfg = SB.cfgs("resnet18")
        shard = {k: v.to(dev) for k, v in shard_batch(ddp_batch(case), rank, world).items()}
        tr = HotPathTrainer(cfg, weights.seeded_state_dict(23 + 100 * rank, **wcfg), dev, world_size=world, sync_bn=True,
                            **DDP_KW)
        losses, grads = [], []
        for i in range(SB.STEPS):
            st = torch.load(os.path.join(out_dir, "ref_state_%d.pt" % i))
            tr.load_state_dict(st["sd"])
            tr.load_optimizer_state_dict(st["opt"])
            loss, _ = tr.forward_backward(shard)
            tr.optimizer_step()
            grads.append(tr.gbucket.flat.clone().cpu())
            losses.append(float(loss))
        m = tr.metrics.read(reduce=True)
        local = tr.metrics.read(reduce=False)
        torch.cuda.synchronize()
        torch.save(dict(losses=losses, grads=grads, sd={k: v.cpu() for k, v in tr.state_dict().items()},
                        metrics=m, local_kept=local["kept"]), os.path.join(out_dir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["uneven", "one_empty"])
def test_two_rank_mean_is_the_mean_over_the_global_batch(tmp_path, case):
    cfg, wcfg = SB.cfgs("resnet18")
    full = {k: v.to(DEV) for k, v in ddp_batch(case).items() if torch.is_tensor(v)}
    ref_tr = HotPathTrainer(cfg, weights.seeded_state_dict(23, **wcfg), DEV, **DDP_KW)
    ref = dict(losses=[], grads=[])
    for i in range(SB.STEPS):
        torch.save(dict(sd={k: v.cpu() for k, v in ref_tr.state_dict().items()},
                        opt={k: (v.cpu() if torch.is_tensor(v) else v)
                             for k, v in ref_tr.optimizer_state_dict().items()}),
                   os.path.join(str(tmp_path), "ref_state_%d.pt" % i))
        loss, _ = ref_tr.forward_backward(full)
        ref["grads"].append(ref_tr.gbucket.flat.clone().cpu())
        ref_tr.optimizer_step()
        ref["losses"].append(float(loss))
    ref["sd"] = {k: v.cpu() for k, v in ref_tr.state_dict().items()}
    ref["offsets"] = ref_tr.gbucket.offsets
    ref_metrics = ref_tr.metrics.read()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    mp.spawn(_ddp_worker, args=(2, free_port(), str(tmp_path), case), nprocs=2, join=True)
    r0, r1 = [torch.load(os.path.join(str(tmp_path), "r%d.pt" % r), weights_only=False) for r in range(2)]
    print("%s: losses rank 0 %s rank 1 %s single process %s; kept per rank %d / %d"
          % (case, r0["losses"], r1["losses"], ref["losses"], r0["local_kept"], r1["local_kept"]))
    assert r0["local_kept"] != r1["local_kept"] and (case == "uneven" or r1["local_kept"] == 0)
    # each rank returns the GLOBAL mean: every rank's loss is held to _check_syncbn's 2e-4 on its own (the helper adds
    # the two ranks' losses, so it is given one rank's and zeros), gradients and parameters to its own bounds
    zeros = [0.0] * SB.STEPS
    SB.check_syncbn(r0, dict(r1, losses=zeros), ref, "resnet18")
    SB.check_syncbn(dict(r0, losses=r1["losses"]), dict(r1, losses=zeros), ref, "resnet18")
    for r in (r0, r1):
        m = r["metrics"]
        assert m["confusion"].tolist() == ref_metrics["confusion"].tolist()
        assert (m["kept"], m["bad_labels"]) == (ref_metrics["kept"], ref_metrics["bad_labels"])
        assert abs(m["loss"] - ref_metrics["loss"]) <= 2e-4 * abs(ref_metrics["loss"])


# ------------------------------------------------------------------------------------------------- module
def test_module_equals_the_c_abi_and_torch():
    nc = 4
    w = class_weights(nc)
    for kw in (dict(), dict(weight=w, label_smoothing=0.1), dict(weight=w, reduction="sum", ignore_index=-1),
               dict(focal_gamma=2.0, weight=w)):
        ig = kw.get("ignore_index", -100)
        logits, labels = make(1440, nc, 50, ig)
        crit = CrossEntropyLoss(**kw).to(DEV)
        lg = logits.to(DEV).requires_grad_(True)
        loss = crit(lg, labels.to(DEV))
        loss.backward()
        ckw = dict(weight=kw.get("weight"), label_smoothing=kw.get("label_smoothing", 0.0),
                   focal_gamma=kw.get("focal_gamma", 0.0), ignore_index=ig, reduction=kw.get("reduction", "mean"))
        _, _, loss_c, dl_c = run(logits, labels, **ckw)
        assert loss.dim() == 0 and torch.equal(loss.detach(), loss_c[0]) and torch.equal(lg.grad, dl_c)
        loss_ref, dl_ref = LO.loss_and_dlogits(logits, labels, **ckw)
        assert abs(loss.item() - float(loss_ref)) <= LOSS_GATE * abs(float(loss_ref))
        close(lg.grad, dl_ref, GRAD_GATE, describe(kw))
        lg3 = logits.to(DEV).requires_grad_(True)
        (crit(lg3, labels.to(DEV)) * 3).backward()
        close(lg3.grad, 3 * dl_ref, GRAD_GATE, "3 x " + describe(kw))
        assert not torch.equal(lg3.grad, lg.grad)


def test_module_drives_one_dropin_step():
    torch.manual_seed(0)
    m = CoVA((3, 3), 64, 4, True, 32, 16, 0, 0.0, None).to(DEV)
    batch = synthetic.make_batch(2, img_h=64, boxes_per_page=[12, 17], context_size=4, seed=5)
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0, 3.0, 3.0]), label_smoothing=0.05).to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    labels = batch["labels"].to(DEV)
    out = m(*args)
    loss = crit(out, labels)
    ref = LO.criterion(out.detach().cpu().double(), batch["labels"], weight=[1.0, 3.0, 3.0, 3.0], label_smoothing=0.05,
                       reduction="mean")
    assert abs(loss.item() - float(ref)) <= LOSS_GATE * abs(float(ref))
    opt.zero_grad()
    loss.backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)
    opt.step()
    assert crit(m(*args), labels).item() != loss.item()
