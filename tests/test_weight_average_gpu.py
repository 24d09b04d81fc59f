"""Weight averaging on the GPU: cova_weight_average bit for bit against the numpy statement (tests/average_oracle.py)
over a ragged table, HotPathTrainer(average=) step by step against the oracle applied to snapshots of the live bucket,
the launches of an averaging step, evaluation on the averaged model and fit(use_average=True) against the same loop
written out by hand.  Every comparison is bit-equal: each operation of the update is one correctly rounded float32
operation, and the schedule is host doubles."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import average_oracle as AO  # noqa: E402
from helpers import bits, DEV, HARD_RAGGED as RAGGED, N_BACKING, N_RAGGED, profiled, ragged_inside, seg_table  # noqa: E402
from config_cases import SPLIT_CFG as ECFG, TRAINER_CFG as CFG  # noqa: E402
from trainer_cases import device_setup as trainer_setup, page_set  # noqa: E402

SENTINEL = 0x7FC12345                      # a NaN with a payload: any arithmetic on it, or any store over it, shows

# RAGGED is the hard ragged table of tests/helpers.py (the malformed row's [8900, 9000) keeps the sentinel)


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    gen = torch.Generator().manual_seed(21)
    inside = ragged_inside()
    avg = torch.randn(N_BACKING, generator=gen)
    p = avg + 0.1 * torch.randn(N_BACKING, generator=gen)
    p[5:40] = avg[5:40]                                       # some unchanged parameters: the fixed point
    avg = torch.where(inside, avg, torch.full((), SENTINEL, dtype=torch.int32).view(torch.float32))
    return avg, p, inside


def weight_average(avg, p, n, seg, n_seg, total, w):
    engine.call("cova_weight_average", avg, p, n, seg, n_seg, total, w)


@pytest.mark.parametrize("w", [0.0, 1.0, 1.0 / 3.0, 1e-3])
def test_kernel_equals_the_numpy_statement_bit_for_bit(w):
    avg0, p0, inside = ragged_inputs()
    seg, total = seg_table(RAGGED)
    assert total == 8889 and total <= N_RAGGED               # (the malformed row's 200 elements count in the table)
    avg, again, p = avg0.to(DEV), avg0.to(DEV), p0.to(DEV)
    weight_average(avg, p, N_RAGGED, seg, len(RAGGED), total, w)
    weight_average(again, p, N_RAGGED, seg, len(RAGGED), total, w)
    torch.cuda.synchronize()
    ref = np.concatenate([AO.average_update(avg0.numpy()[:N_RAGGED], p0.numpy()[:N_RAGGED], RAGGED, w),
                          avg0.numpy()[N_RAGGED:]])
    got = bits(avg)
    assert torch.equal(got, bits(ref))
    assert torch.equal(got, bits(again))                                      # a rerun gives the same bits
    assert bool((got[~inside] == SENTINEL).all())                             # gaps, tail, the malformed row, past n
    assert torch.equal(bits(p), bits(p0))
    changed = got != bits(avg0)
    if w == 0.0:
        assert not changed.any()                                              # the average unchanged, bit for bit
    else:
        assert not changed[5:40].any() and changed[inside].float().mean() > 0.9   # p == avg is a fixed point
    if w == 1.0:
        assert float((avg.cpu()[inside] - p0[inside]).abs().max()) <= 1e-6       # avg + (p - avg): p up to one rounding


def test_no_rows_or_no_elements_launch_nothing():
    avg0, p0, _ = ragged_inputs()
    avg, p = avg0.to(DEV), p0.to(DEV)
    seg, total = seg_table(RAGGED)
    for n_seg, tot in ((0, total), (len(RAGGED), 0), (0, 0)):
        weight_average(avg, p, N_RAGGED, seg, n_seg, tot, 0.5)
    weight_average(avg, p, N_RAGGED, seg[:0], 0, 0, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(bits(avg), bits(avg0))
    with pytest.raises(_lib.CovaHipError):                                    # more table elements than the buffer has
        weight_average(avg, p, 100, seg, len(RAGGED), total, 0.5)
    assert torch.equal(bits(avg), bits(avg0))


# ---------------------------------------------------------------------------------------------- the trainer
FROZEN = ("convnet.0.", "convnet.1.")
STEPS = 6


@functools.lru_cache(maxsize=None)
def plain_run(frozen):
    """STEPS steps of the trainer without averaging -> per step (loss, parameters, moments), computed once."""
    sd, batches = trainer_setup()
    tr = HotPathTrainer(CFG, sd, DEV, frozen=frozen)
    out = []
    for it in range(STEPS):
        loss, _ = tr.train_step(batches[it % 3])
        out.append((loss.clone(), tr.pbucket.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    return out, tr.state_dict()


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


@pytest.mark.parametrize("frozen", [(), FROZEN])
@pytest.mark.parametrize("kind, kw", [("ema", dict(average_decay=0.9, average_warmup=3)),
                                      ("swa", dict(average_start=2, average_every=2))])
def test_trajectory_follows_the_oracle_and_leaves_training_alone(kind, kw, frozen):
    sd, batches = trainer_setup()
    ref_steps, ref_sd = plain_run(frozen)
    tr = HotPathTrainer(CFG, sd, DEV, frozen=frozen, average=kind, **kw)
    a = tr.average
    rows = trainable_rows(tr)
    assert bool(tr.frozen) == bool(frozen) and rows[0][0] == (0 if not frozen else tr.pbucket.offsets["convnet.4.0.conv1.weight"][0])
    actions, n_end = AO.schedule(kind, a.decay, a.warmup, a.start, a.every, STEPS)
    assert sum(isinstance(x, float) for x in actions) >= 2
    nb = tr.bbucket.flat.numel()
    avg = tr.pbucket.flat.cpu().numpy() if a.start == 0 else None            # start 0: a copy at construction
    bavg = tr.bbucket.flat.cpu().numpy() if a.start == 0 else None
    tracked = tr.tracked.cpu() if a.start == 0 else None
    for it, action in enumerate(actions):
        loss, _ = tr.train_step(batches[it % 3])
        # averaging does not perturb training: losses, parameters and moments are those of the plain trainer
        for got, want in zip((loss, tr.pbucket.flat, tr.exp_avg, tr.exp_avg_sq), ref_steps[it]):
            assert torch.equal(bits(got), bits(want)), it
        p, b = tr.pbucket.flat.cpu().numpy(), tr.bbucket.flat.cpu().numpy()
        if action == "copy":
            avg, bavg, tracked = p.copy(), b.copy(), tr.tracked.cpu()
        elif action is not None:
            avg = AO.average_update(avg, p, rows, action)
            bavg = AO.average_update(bavg, b, [(0, nb)], action)
            tracked = tr.tracked.cpu()                                        # copied, not averaged
        if avg is None:
            assert tr.n_averaged == 0
            continue
        assert torch.equal(bits(tr.abucket.flat), bits(avg)), it
        assert torch.equal(bits(tr.abbucket.flat), bits(bavg)), it
        assert torch.equal(tr.atracked.cpu(), tracked), it
    assert tr.average.n_averaged == n_end
    assert not torch.equal(tr.abucket.flat, tr.pbucket.flat) and not torch.equal(tr.abbucket.flat, tr.bbucket.flat)
    got, live = tr.averaged_state_dict(), tr.state_dict()
    for k in live:                                                            # the live model ends where the plain one does
        assert torch.equal(live[k], ref_sd[k]), k
    for k in tr.frozen:                                                       # frozen tensors never drift
        assert torch.equal(got[k], live[k]) and torch.equal(got[k].cpu(), sd[k]), k


def test_averaging_step_adds_its_launches_and_no_host_synchronisation():
    sd, batches = trainer_setup()
    for kw in (dict(), dict(frozen=FROZEN), dict(optimizer="adamw", max_grad_norm=1.0)):   # plain, per-run and fused steps
        plain = HotPathTrainer(CFG, sd, DEV, **kw)
        plain.forward_backward(batches[0])
        base = profiled(plain.optimizer_step)[1]
        assert "cova_weight_average" not in base
        for buffers in (True, False):
            tr = HotPathTrainer(CFG, sd, DEV, average="ema", average_buffers=buffers, **kw)
            tr.forward_backward(batches[0])
            prof = profiled(tr.optimizer_step)[1]
            assert prof == dict(base, cova_weight_average=2 if buffers else 1), (kw, buffers, prof)
    # steps 1 (before the start), 2 (the copy) and 3, 4 (updates): none reads anything back
    tr = HotPathTrainer(CFG, sd, DEV, average="swa", average_start=2)
    for it in range(4):
        tr.forward_backward(batches[it % 3])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tr.optimizer_step()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    assert tr.n_averaged == 3


# ---------------------------------------------------------------------------------------------- evaluation and fit
CS = 6


@functools.lru_cache(maxsize=None)
def splits():
    u8, rows = page_set(9)
    v8, vrows = page_set(20, seed=9)
    sd = weights.seeded_state_dict(77, logit_gain=2.0, **{k: v for k, v in ECFG.items() if k != "drop_prob"})
    return DeviceDataset(u8, rows, CS, DEV), DeviceDataset(v8, vrows, CS, DEV), sd


@pytest.mark.parametrize("buffers", [True, False])
def test_averaged_weights_run_the_averaged_model_without_a_copy(buffers):
    train, val, sd = splits()
    tr = HotPathTrainer(ECFG, sd, DEV, lr=2e-3, average="ema", average_decay=0.5, average_buffers=buffers)
    for batch in train.batches(3, shuffle=True, sampling_fraction=0.9, seed=5, epoch=1):
        tr.train_step(batch)
    assert tr.n_averaged == 4
    batch = next(iter(val.batches(5)))
    before, _ = tr.predict(batch)
    fresh = HotPathTrainer(ECFG, tr.averaged_state_dict(), DEV)
    want, _ = fresh.predict(batch)
    want_rep = evaluate_split(fresh, val, batch_size=5)
    ptr = tr.abucket.flat.data_ptr()
    with tr.averaged_weights():
        inside, _ = tr.predict(batch)
        rep = evaluate_split(tr, val, batch_size=5)
        assert tr.params["convnet.0.weight"].data_ptr() == tr.abucket.views["convnet.0.weight"].data_ptr()
    assert tr.abucket.flat.data_ptr() == ptr
    after, _ = tr.predict(batch)
    assert torch.equal(bits(inside), bits(want)) and not torch.equal(inside, before)
    assert torch.equal(bits(after), bits(before))
    assert np.array_equal(rep.ranks, want_rep.ranks) and np.array_equal(rep.top1, want_rep.top1)
    live_rep = evaluate_split(tr, val, batch_size=5)
    assert live_rep.evaluated.all() and rep.evaluated.all()
    loss, _ = tr.train_step(batch)                                            # and training goes on afterwards
    assert tr.n_averaged == 5 and bool(torch.isfinite(loss).all())


def hand_loop(tr, train, val, n_epochs, bs, sf, seed, interval, k):
    """fit(use_average=True) written out from train_step, metrics.read, averaged_weights and averaged_state_dict."""
    best, best_state, best_epoch, history = 0.0, None, None, []
    tr.metrics.reset()
    for epoch in range(1, n_epochs + 1):
        for batch in train.batches(bs, shuffle=True, sampling_fraction=sf, seed=seed, epoch=epoch):
            tr.train_step(batch)
        m = tr.metrics.read()
        tr.metrics.reset()
        rec = dict(loss=m["loss_numerator"] / m["kept"], accuracy=100.0 * np.trace(m["confusion"]) / m["kept"],
                   boxes=m["kept"], eval_acc=None, averaged=False, is_best=False)
        history.append(rec)
        if epoch == 1 or epoch % interval == 0 or epoch == n_epochs:
            if tr.average.n_averaged > 0:
                rec["averaged"] = True
                with tr.averaged_weights():
                    report = evaluate_split(tr, val)
            else:
                report = evaluate_split(tr, val)
            rec["eval_acc"] = float(report.class_acc(k)[1:].mean())
            if rec["eval_acc"] > best:
                best, best_epoch, rec["is_best"] = rec["eval_acc"], epoch, True
                best_state = tr.averaged_state_dict() if rec["averaged"] else tr.state_dict()
    if best_state is not None:
        tr.load_state_dict(best_state)
    return best, best_epoch, best_state, history


FIT = dict(sampling_fraction=0.9, seed=12, eval_interval=2, k=3)
KEYS = ("loss", "accuracy", "boxes", "eval_acc", "averaged", "is_best")


def test_fit_with_use_average_equals_the_loop_written_out_by_hand(tmp_path):
    train, val, sd = splits()
    # 3 steps per epoch; the average starts at step 4, so the evaluation of epoch 1 runs on the live weights
    kw = dict(lr=2e-3, track_metrics=True, average="ema", average_decay=0.8, average_start=4)
    a, b = (HotPathTrainer(ECFG, sd, DEV, **kw) for _ in range(2))
    ckpt = str(tmp_path / "best.pth")
    res = fit(a, train, val, 4, 3, checkpoint=ckpt, use_average=True, **FIT)
    best, best_epoch, best_state, history = hand_loop(b, train, val, 4, 3, FIT["sampling_fraction"], FIT["seed"],
                                                      FIT["eval_interval"], FIT["k"])
    assert res.epochs_run == 4 and (res.best_eval_acc, res.best_epoch) == (best, best_epoch) and best_epoch is not None
    for got, ref in zip(res.history, history):
        for key in KEYS:
            assert got[key] == ref[key], (got["epoch"], key)
    assert [h["averaged"] for h in res.history] == [False, True, False, True]
    assert [h["eval_acc"] is not None for h in res.history] == [True, True, False, True]
    # live parameters and the average both hold the best state, which is the saved one; the trajectory behind it is equal
    saved, now, avg = torch.load(ckpt, map_location=DEV), a.state_dict(), a.averaged_state_dict()
    assert list(saved) == list(now) == list(best_state) == list(avg)
    for key in now:
        assert torch.equal(bits(now[key]), bits(saved[key])) and torch.equal(bits(now[key]), bits(best_state[key])), key
        assert torch.equal(bits(avg[key]), bits(now[key])), key
    assert torch.equal(a.pbucket.flat, b.pbucket.flat) and torch.equal(a.abucket.flat, b.abucket.flat)
    assert torch.equal(a.exp_avg, b.exp_avg) and a.step_count == b.step_count == 12
    assert a.average.n_averaged == b.average.n_averaged == 1                  # restarted by the final reload


def test_fit_without_use_average_is_the_plain_loop_and_refuses_a_plain_trainer():
    train, val, sd = splits()
    kw = dict(lr=2e-3, track_metrics=True)
    plain, averaging = HotPathTrainer(ECFG, sd, DEV, **kw), HotPathTrainer(ECFG, sd, DEV, average="swa", **kw)
    with pytest.raises(ValueError, match="average="):
        fit(plain, train, val, 1, 3, use_average=True, **FIT)
    assert plain.step_count == 0
    ref = fit(plain, train, val, 3, 3, **FIT)
    res = fit(averaging, train, val, 3, 3, use_average=False, **FIT)
    assert (res.best_eval_acc, res.best_epoch, res.epochs_run, res.stopped_early) == \
        (ref.best_eval_acc, ref.best_epoch, ref.epochs_run, ref.stopped_early)
    for got, want in zip(res.history, ref.history):
        assert not got["averaged"] and not want["averaged"]
        for key in KEYS:
            assert got[key] == want[key], (got["epoch"], key)
    a, b = averaging.state_dict(), plain.state_dict()
    for key in a:
        assert torch.equal(bits(a[key]), bits(b[key])), key
