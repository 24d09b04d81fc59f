"""Gradient accumulation on the GPU: cova_grad_accumulate bit for bit against the numpy statement
(tests/accumulate_oracle.py) over a ragged table, every clip and both alignments; HotPathTrainer(accumulate_steps=)
update by update against the cycle written out by hand on a plain trainer; the launches of a micro-step; the clipped
two-launch close of the overlapped exchange on a 1-rank group; two accumulated half batches against the whole batch; and
fit() against the loop written out by hand.  Every comparison but the half-batch one is bit-equal: each operation of the
kernel is one correctly rounded float32 operation in a fixed order, and the schedule is host integers."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, evaluation, synthetic, weights  # noqa: E402
from cova_web_object_detection_amd import trainer as T  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import accumulate_oracle as GO  # noqa: E402
from helpers import (bits, DEV, HARD_RAGGED as RAGGED, N_BACKING,  # noqa: E402
                     N_RAGGED, on_device, profiled, ragged_inside, seg_table)
from config_cases import SPLIT_CFG as ECFG, TRAINER_CFG as CFG  # noqa: E402
from trainer_cases import device_setup as trainer_setup, page_set  # noqa: E402

SENTINEL = 0x7FC12345                      # a NaN with a payload: any arithmetic on it, or any store over it, shows
GARBAGE = 0x7FC0BEEF                       # what an accumulator holds before its first cycle

# RAGGED is the hard ragged table of tests/helpers.py (the malformed row's [8900, 9000) keeps the sentinel).  The clips: the
# full range; an unaligned start inside row (3005, 3007) and an end inside row (6600, 8800); an empty clip
CLIPS = {"full": (0, N_RAGGED), "cut": (3006, 7001), "empty": (5000, 5000)}


def pattern(x):
    return torch.full((), x, dtype=torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    gen = torch.Generator().manual_seed(33)
    inside = ragged_inside()
    acc = torch.where(inside, torch.randn(N_BACKING, generator=gen), pattern(SENTINEL))
    g = torch.where(inside, 0.3 * torch.randn(N_BACKING, generator=gen), pattern(SENTINEL))
    return acc, g, inside


def accumulate(mode, acc, g, n, seg, n_seg, total, clip, scale):
    engine.call("cova_grad_accumulate", mode, acc, g, n, seg, n_seg, total, clip[0], clip[1], scale)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("mode", list(GO.MODES))
def test_kernel_equals_the_numpy_statement_bit_for_bit(mode, clip, offset):
    acc0, g0, inside = ragged_inputs()
    if mode == GO.OPEN:                                      # open never reads acc: garbage in it leaves no trace
        acc0 = torch.where(inside, pattern(GARBAGE), acc0)
    seg, total = seg_table(RAGGED)
    assert total == 8889 and total <= N_RAGGED               # (the malformed row's 200 elements count in the table)
    c0, c1 = CLIPS[clip]
    touched = inside.clone()
    touched[:c0] = False
    touched[c1:] = False
    for scale in (1.0, 0.5, 1.0 / 3.0):
        acc, g = on_device(acc0, offset), on_device(g0, offset)
        acc2, g2 = on_device(acc0, offset), on_device(g0, offset)
        accumulate(mode, acc, g, N_RAGGED, seg, len(RAGGED), total, (c0, c1), scale)
        accumulate(mode, acc2, g2, N_RAGGED, seg, len(RAGGED), total, (c0, c1), scale)
        torch.cuda.synchronize()
        want_acc, want_g = GO.accumulate(mode, acc0.numpy()[:N_RAGGED], g0.numpy()[:N_RAGGED], RAGGED, scale, (c0, c1))
        want_acc = np.concatenate([want_acc, acc0.numpy()[N_RAGGED:]])
        want_g = np.concatenate([want_g, g0.numpy()[N_RAGGED:]])
        got_acc, got_g = bits(acc), bits(g)
        assert torch.equal(got_acc, bits(want_acc)) and torch.equal(got_g, bits(want_g)), scale
        assert torch.equal(got_acc, bits(acc2)) and torch.equal(got_g, bits(g2))          # a rerun gives the same bits
        # outside rows or clip every element keeps its bits in both buffers: the sentinel in gaps, tail, the malformed
        # row and past n, the old values in the rows the clip cut off
        assert torch.equal(got_acc[~touched], bits(acc0)[~touched]) and torch.equal(got_g[~touched], bits(g0)[~touched])
        assert bool((got_acc[~inside] == SENTINEL).all()) and bool((got_g[~inside] == SENTINEL).all())
        if mode in (GO.OPEN, GO.ADD):                        # the read-only operand
            assert torch.equal(got_g, bits(g0))
        else:
            assert torch.equal(got_acc, bits(acc0))
        if touched.any():
            changed = (got_acc != bits(acc0)) | (got_g != bits(g0))
            assert changed[touched].float().mean() > 0.9 and bool(torch.isfinite((acc if mode < 2 else g).cpu()[touched]).all())
        if scale == 1.0 and mode == GO.ADD_CLOSE:            # the plain float32 sum
            assert torch.equal(g.cpu()[touched], (acc0 + g0)[:N_BACKING][touched])
    assert touched.sum() == {"full": 8689, "cut": 1 + 3487 + 401, "empty": 0}[clip]


def test_no_launch_and_error_cases():
    acc0, g0, _ = ragged_inputs()
    acc, g = acc0.to(DEV), g0.to(DEV)
    seg, total = seg_table(RAGGED)
    for mode in GO.MODES:
        for n_seg, tot in ((0, total), (len(RAGGED), 0), (0, 0)):
            accumulate(mode, acc, g, N_RAGGED, seg, n_seg, tot, (0, N_RAGGED), 0.5)
        accumulate(mode, acc, g, N_RAGGED, seg[:0], 0, 0, (0, N_RAGGED), 0.5)
        accumulate(mode, acc, g, N_RAGGED, seg, len(RAGGED), total, (7001, 3006), 0.5)     # a reversed clip is empty
        with pytest.raises(_lib.CovaHipError):               # more table elements than the buffer has
            accumulate(mode, acc, g, 100, seg, len(RAGGED), total, (0, 100), 0.5)
    with pytest.raises(_lib.CovaHipError):                   # no such mode
        accumulate(4, acc, g, N_RAGGED, seg, len(RAGGED), total, (0, N_RAGGED), 0.5)
    torch.cuda.synchronize()
    assert torch.equal(bits(acc), bits(acc0)) and torch.equal(bits(g), bits(g0))
    # a clip beyond the buffer is clamped to it
    accumulate(GO.ADD, acc, g, N_RAGGED, seg, len(RAGGED), total, (-50, 1 << 40), 1.0)
    torch.cuda.synchronize()
    want, _ = GO.accumulate(GO.ADD, acc0.numpy()[:N_RAGGED], g0.numpy()[:N_RAGGED], RAGGED)
    assert torch.equal(bits(acc)[:N_RAGGED], bits(want)) and torch.equal(bits(acc)[N_RAGGED:], bits(acc0)[N_RAGGED:])


# ---------------------------------------------------------------------------------------------- the trainer
FROZEN = ("convnet.0.", "convnet.1.")


def trainable_rows(tr):
    """Merged runs of the trainable tensors, restated from the bucket layout (a run spans the alignment padding)."""
    keys, n = list(tr.pbucket.offsets), tr.pbucket.flat.numel()
    ends = [tr.pbucket.offsets[k][0] for k in keys[1:]] + [n]
    rows = []
    for k, hi in zip(keys, ends):
        if k.startswith(FROZEN) and tr.frozen:
            continue
        lo = tr.pbucket.offsets[k][0]
        if rows and rows[-1][1] == lo:
            rows[-1] = (rows[-1][0], hi)
        else:
            rows.append((lo, hi))
    return rows


def assert_same_state(a, b, what):
    for name in ("pbucket.flat", "exp_avg", "exp_avg_sq", "gbucket.flat"):
        x, y = functools.reduce(getattr, name.split("."), a), functools.reduce(getattr, name.split("."), b)
        assert torch.equal(bits(x), bits(y)), (what, name)
    for k in a.buffers:                                      # BatchNorm statistics and counters: every micro-batch counts
        assert torch.equal(bits(a.buffers[k]), bits(b.buffers[k])), (what, k)


OPTIONS = {"adam": dict(), "adamw_clip": dict(optimizer="adamw", max_grad_norm=1.0),
           "mean": dict(loss_reduction="mean"), "ema": dict(average="ema", average_decay=0.9)}


@pytest.mark.parametrize("frozen", [(), FROZEN])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("opt", list(OPTIONS))
def test_trainer_follows_the_cycle_written_out_by_hand(opt, n, frozen):
    """n = 2: batches 0, 1 close a cycle, batch 2 is flushed alone (scale 1).  n = 3: batches 0, 1, 2 close a cycle,
    batches 0, 1 are flushed (scale 1/2 with the mean)."""
    sd, batches = trainer_setup()
    kw = dict(OPTIONS[opt], frozen=frozen)
    tr = HotPathTrainer(CFG, sd, DEV, accumulate_steps=n, **kw)
    hand = HotPathTrainer(CFG, sd, DEV, **kw)
    rows = trainable_rows(hand)
    assert tr._acc_seg.cpu()[:, :2].tolist() == [list(r) for r in rows]
    reduction = kw.get("loss_reduction", "sum")
    order = [0, 1, 2] if n == 2 else [0, 1, 2, 0, 1]
    pending, updates, scales = [], 0, []

    def hand_update(flushed):
        nonlocal updates
        updates += 1
        scale = GO.scale_of(reduction, len(pending))
        scales.append(scale)
        g = (GO.flushed_gradient if flushed else GO.accumulated_gradient)(pending, rows, scale)
        hand.gbucket.flat.copy_(torch.from_numpy(g))
        micro, hand.step_count = hand.step_count, updates   # the optimizer's step is the update number
        hand.optimizer_step()
        hand.step_count = micro
        del pending[:]

    for it, b in enumerate(order):
        loss, pred = tr.train_step(batches[b])
        want_loss, want_pred = hand.forward_backward(batches[b])
        assert torch.equal(bits(loss), bits(want_loss)) and torch.equal(pred, want_pred), it
        pending.append(hand.gbucket.flat.cpu().numpy().copy())
        assert tr.step_count == hand.step_count == it + 1
        if len(pending) == n:
            hand_update(False)
            assert_same_state(tr, hand, ("close", it))
        else:                                                # a micro-step changes no parameter and no moment
            for x, y in ((tr.pbucket.flat, hand.pbucket.flat), (tr.exp_avg, hand.exp_avg)):
                assert torch.equal(bits(x), bits(y)), it
        assert (tr.accumulated, tr.update_count) == (len(pending), updates)
    assert tr.accumulated == len(order) - n and tr.flush() is True
    hand_update(True)
    assert_same_state(tr, hand, "flush")
    assert (tr.accumulated, tr.update_count, tr.step_count) == (0, 2, len(order)) and tr.flush() is False
    assert scales == {"sum": [1.0, 1.0], "mean": [1.0 / n, 1.0 / (len(order) - n)]}[reduction]
    if opt == "adamw_clip":
        assert torch.equal(bits(tr.last_grad_norm), bits(hand.last_grad_norm))
    if opt == "ema":                                         # one sample per update, not per micro-step
        assert tr.n_averaged == hand.n_averaged == 3
        assert torch.equal(bits(tr.abucket.flat), bits(hand.abucket.flat))
        assert torch.equal(bits(tr.abbucket.flat), bits(hand.abbucket.flat))
    st = tr.optimizer_state_dict()
    assert (st["step"], st["updates"]) == (len(order), 2)
    now = tr.state_dict()
    for k in tr.frozen:
        assert torch.equal(now[k].cpu(), sd[k]), k
    assert bool(tr.frozen) == bool(frozen) and not torch.equal(tr.pbucket.flat.cpu(), HotPathTrainer(CFG, sd, DEV).pbucket.flat.cpu())


def _recorded(monkeypatch):
    """engine.call with the name and the arguments of every launch recorded in order."""
    calls, real = [], engine.call

    def call(name, *a, **k):
        calls.append((name,) + a)
        return real(name, *a, **k)
    monkeypatch.setattr(engine, "call", call)
    return calls


def test_launch_counts_and_no_host_synchronisation(monkeypatch):
    sd, batches = trainer_setup()
    for kw in (dict(), dict(frozen=FROZEN), dict(optimizer="adamw", max_grad_norm=1.0)):
        parent, one = HotPathTrainer(CFG, sd, DEV, **kw), HotPathTrainer(CFG, sd, DEV, accumulate_steps=1, **kw)
        step = profiled(lambda: parent.train_step(batches[0]))[1]
        assert profiled(lambda: one.train_step(batches[0]))[1] == step and "cova_grad_accumulate" not in step
        assert not hasattr(one, "accbucket") and profiled(one.flush)[1] == {}
        fb = profiled(lambda: parent.forward_backward(batches[0]))[1]
        update = {k: v - fb.get(k, 0) for k, v in step.items() if v != fb.get(k, 0)}     # the optimizer's launches
        tr = HotPathTrainer(CFG, sd, DEV, accumulate_steps=3, **kw)
        for it in range(2):                                  # open, add: the backward's launches and one more
            assert profiled(lambda: tr.train_step(batches[0]))[1] == dict(fb, cova_grad_accumulate=1), (kw, it)
        assert profiled(lambda: tr.train_step(batches[0]))[1] == dict(step, cova_grad_accumulate=1), kw
        assert profiled(tr.flush)[1] == {}                     # nothing pending: nothing launched
        tr.train_step(batches[0])
        assert update and profiled(tr.flush)[1] == dict(update, cova_grad_accumulate=1), kw
    # the order of the closing micro-step: the backward, the one accumulate launch, then the optimizer's launches
    tr = HotPathTrainer(CFG, sd, DEV, accumulate_steps=2, optimizer="adamw", max_grad_norm=1.0)
    calls = _recorded(monkeypatch)
    tr.train_step(batches[0])
    tr.train_step(batches[1])
    names = [c[0] for c in calls]
    assert names.count("cova_grad_accumulate") == 2 and names[-3:] == ["cova_grad_accumulate", "cova_grad_norm", "cova_optim_step"]
    assert [c[1] for c in calls if c[0] == "cova_grad_accumulate"] == [GO.OPEN, GO.ADD_CLOSE]
    monkeypatch.undo()
    # no micro-step reads anything back: what train_step() and flush() add to forward_backward() runs under the guard
    tr = HotPathTrainer(CFG, sd, DEV, accumulate_steps=3, average="swa", average_start=1, max_grad_norm=1.0)
    inner = tr.forward_backward

    def forward_backward(batch, masks=None):
        torch.cuda.set_sync_debug_mode(0)
        try:
            return inner(batch, masks)
        finally:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
    tr.forward_backward = forward_backward
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in range(5):
            tr.train_step(batches[it % 3])
        assert tr.flush() is True
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert (tr.update_count, tr.step_count, tr.n_averaged) == (2, 5, 2)


def test_one_rank_group_closes_head_and_conv_ranges_separately(monkeypatch):
    """The exchange path with a 1-rank RCCL group (the construction of tests/test_model_gpu.py): the sums are
    identities, so the overlapped close in two clipped launches must give the single-process trainer's bits."""
    import os
    import socket
    import torch.distributed as dist
    sd, batches = trainer_setup()
    assert engine.OPTIONS.overlap_allreduce
    ref = HotPathTrainer(CFG, sd, DEV, accumulate_steps=2, max_grad_norm=1.0)
    for it in range(5):
        ref.train_step(batches[it % 3])
    ref.flush()
    collectives = []
    for name in ("all_reduce_range", "all_reduce_sum"):
        def counted(self, *a, _real=getattr(T.FlatBucket, name), _name=name, **k):
            collectives.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(T.FlatBucket, name, counted)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        tr = HotPathTrainer(CFG, sd, DEV, world_size=2, accumulate_steps=2, max_grad_norm=1.0)   # world_size > 1: exchange on
        calls = _recorded(monkeypatch)
        head, numel = tr._head_offset(), tr.gbucket.flat.numel()
        assert 0 < head < numel
        for it in range(5):
            del calls[:], collectives[:]
            tr.train_step(batches[it % 3])
            acc = [(c[1], c[8], c[9]) for c in calls if c[0] == "cova_grad_accumulate"]
            if it % 2 == 0:                                  # a micro-step: one launch, no collective
                assert acc == [(GO.OPEN, 0, numel)] and collectives == [], it
            else:                                            # the head closes under the backward, the conv stack after it
                assert acc == [(GO.ADD_CLOSE, head, numel), (GO.ADD_CLOSE, 0, head)], it
                assert collectives == ["all_reduce_range", "all_reduce_range"], it
        del calls[:], collectives[:]
        assert tr.flush() is True                            # no overlap to be had: one close, one all-reduce
        assert [(c[1], c[8], c[9]) for c in calls if c[0] == "cova_grad_accumulate"] == [(GO.CLOSE, 0, numel)]
        assert collectives == ["all_reduce_sum"]
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert_same_state(tr, ref, "one rank")
    assert torch.equal(bits(tr.last_grad_norm), bits(ref.last_grad_norm)) and tr.update_count == ref.update_count == 3


def test_two_accumulated_halves_are_the_whole_batch():
    """loss_reduction="sum", no dropout and every BatchNorm in eval mode (bn_eval accepts all of them: the conv stack's,
    bbox_feat_encoder.1 and decoder.2): pages are independent, so the gradient of a 4-page batch is the sum of the
    gradients of its two halves and differs from it by f32 re-association inside the reductions only.  The bounds are
    those tests/test_syncbn_gpu.py::_check_syncbn applies to two ranks against the concatenated batch (quantiles of
    |d| / scale over every 7th element, and the maximum), near-tie gate flips included."""
    sd, _ = trainer_setup()
    batch = synthetic.make_batch(4, img_h=96, boxes_per_page=[20, 11, 23, 13], context_size=6, seed=905)
    kw = dict(bn_eval=("convnet.", "bbox_feat_encoder.1.", "decoder.2."), max_grad_norm=1e9)
    whole, tr = HotPathTrainer(CFG, sd, DEV, **kw), HotPathTrainer(CFG, sd, DEV, accumulate_steps=2, **kw)
    assert isinstance(tr.modes, dict) and len(tr.modes) == sum(k.endswith("running_mean") for k in tr.buffers)
    loss_ref, _ = whole.train_step({k: v.to(DEV) for k, v in batch.items() if torch.is_tensor(v)})
    losses = []
    for r in range(2):
        half = T.shard_batch(batch, r, 2)
        losses.append(tr.train_step({k: v.to(DEV) for k, v in half.items() if torch.is_tensor(v)})[0])
    assert tr.accumulated == 0 and tr.update_count == 1
    tot, ref = float(losses[0]) + float(losses[1]), float(loss_ref)
    assert abs(tot - ref) <= 2e-4 * abs(ref), (tot, ref)
    g_ref = whole.gbucket.flat
    scale = float(g_ref.abs().max())
    d = (tr.gbucket.flat - g_ref).double().abs()
    q = tuple(float(torch.quantile(d[::7].float(), p_)) / scale for p_ in (0.5, 0.9, 0.99, 0.999))
    print("accumulate halves: |d|/scale quantiles 0.5 %.2e  0.9 %.2e  0.99 %.2e  0.999 %.2e  max %.2e"
          % (q + (float(d.max()) / scale,)))
    print("accumulate halves: grad norm %.6e against %.6e" % (float(tr.last_grad_norm), float(whole.last_grad_norm)))
    assert scale > 0 and q[0] <= 1e-6 and q[1] <= 2e-4, q
    assert q[3] <= 1e-3, q
    assert float(d.max()) <= 1e-2 * scale, float(d.max()) / scale
    for k, v in whole.buffers.items():                       # eval mode: no statistic moved, in either trainer
        assert torch.equal(v.cpu(), sd[k]) and torch.equal(tr.buffers[k].cpu(), sd[k]), k


# ---------------------------------------------------------------------------------------------- fit
CS = 6


def hand_loop(tr, train, val, n_epochs, bs, sf, seed, interval, k, lr_schedule):
    """fit() written out from train_step, flush, metrics.read and evaluate_split."""
    best, best_state, best_epoch, history = 0.0, None, None, []
    base_lr = [g["lr"] for g in tr.param_groups]
    tr.metrics.reset()
    for epoch in range(1, n_epochs + 1):
        first = tr.update_count
        for batch in train.batches(bs, shuffle=True, sampling_fraction=sf, seed=seed, epoch=epoch):
            tr.train_step(batch)
        tr.flush()
        m = tr.metrics.read()
        tr.metrics.reset()
        rec = dict(loss=m["loss_numerator"] / m["kept"], accuracy=100.0 * np.trace(m["confusion"]) / m["kept"],
                   boxes=m["kept"], eval_acc=None, is_best=False, updates=tr.update_count - first,
                   lr=[g["lr"] for g in tr.param_groups])
        history.append(rec)
        if epoch == 1 or epoch % interval == 0 or epoch == n_epochs:
            assert tr.accumulated == 0
            rec["eval_acc"] = float(evaluate_split(tr, val).class_acc(k)[1:].mean())
            if rec["eval_acc"] > best:
                best, best_epoch, rec["is_best"] = rec["eval_acc"], epoch, True
                best_state = tr.state_dict()
        for g, lr in zip(tr.param_groups, base_lr):
            g["lr"] = lr * lr_schedule(epoch)
    if best_state is not None:
        tr.load_state_dict(best_state)
    return best, best_epoch, history


def test_fit_equals_the_loop_written_out_by_hand(monkeypatch):
    u8, rows = page_set(9)
    v8, vrows = page_set(20, seed=9)
    sd = weights.seeded_state_dict(77, logit_gain=2.0, **{k: v for k, v in ECFG.items() if k != "drop_prob"})
    train, val = DeviceDataset(u8, rows, CS, DEV), DeviceDataset(v8, vrows, CS, DEV)
    kw = dict(lr=2e-3, track_metrics=True, accumulate_steps=2)
    a, b = (HotPathTrainer(ECFG, sd, DEV, **kw) for _ in range(2))
    n_batches = len(list(train.batches(3, shuffle=True, sampling_fraction=0.9, seed=12, epoch=1)))
    assert n_batches == 3                                    # an odd number: every epoch ends with a flush of one
    schedule = lambda epoch: 0.5 ** epoch                    # noqa: E731
    at_evaluation, real = [], evaluation.evaluate_split

    def checked(trainer, dataset, **k):
        at_evaluation.append(trainer.accumulated)
        return real(trainer, dataset, **k)
    monkeypatch.setattr(evaluation, "evaluate_split", checked)
    res = fit(a, train, val, 3, 3, sampling_fraction=0.9, seed=12, eval_interval=2, k=3, lr_schedule=schedule)
    monkeypatch.undo()
    best, best_epoch, history = hand_loop(b, train, val, 3, 3, 0.9, 12, 2, 3, schedule)
    assert at_evaluation == [0, 0, 0]
    assert res.epochs_run == 3 and (res.best_eval_acc, res.best_epoch) == (best, best_epoch)
    for got, ref in zip(res.history, history):
        for key in ("loss", "accuracy", "boxes", "eval_acc", "is_best", "updates", "lr"):
            assert got[key] == ref[key], (got["epoch"], key)
        assert got["updates"] == math.ceil(n_batches / 2) == 2
    now, want = a.state_dict(), b.state_dict()
    for key in now:
        assert torch.equal(bits(now[key]), bits(want[key])), key
    for x, y in ((a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (a.gbucket.flat, b.gbucket.flat)):
        assert torch.equal(bits(x), bits(y))
    assert a.step_count == b.step_count == 9 and a.update_count == b.update_count == 6 and a.accumulated == 0
