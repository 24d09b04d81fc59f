"""Host logic of gradient accumulation (no GPU): the numpy statement of cova_grad_accumulate on hand-written vectors, the
cycle schedule, the exported entry point, option checks, what the default leaves as before, the launches of a cycle with
the launch recorded instead of issued, the state-dict rules, the counters across two gloo ranks and fit()'s flush at the
end of an epoch."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import cova_amd  # noqa: E402,F401

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

import accumulate_oracle as GO  # noqa: E402
from cova_web_object_detection_amd import _lib, evaluation, weights  # noqa: E402
from cova_web_object_detection_amd import trainer as T  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from config_cases import BASE as CFG, spec_of  # noqa: E402
from helpers import free_port  # noqa: E402

WCFG = spec_of(CFG)
SD = weights.seeded_state_dict(3, **WCFG)
FROZEN = ("convnet.0.", "convnet.1.")


def trainer(sd=SD, **kw):
    return HotPathTrainer(CFG, sd, "cpu", **kw)


def f32(*x):
    return np.asarray(x, dtype=np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


# ---------------------------------------------------------------- 1. the numpy statement of the four modes
G = f32(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
ACC = f32(0.5, 0.25, 1e8, -4, 0.1, 0.2, 0.3, 0.4, 100, 200)
ROWS = [(1, 4), (4, 4), (6, 9), (8, 12), (-1, 2)]          # two rows, an empty one, two malformed ones (skipped)


def test_modes_on_hand_written_vectors():
    acc, g = GO.accumulate(GO.OPEN, ACC, G, ROWS)
    assert same_bits(acc, f32(0.5, 2, 3, 4, 0.1, 0.2, 7, 8, 9, 200)) and same_bits(g, G)
    acc, g = GO.accumulate(GO.ADD, ACC, G, ROWS)
    assert same_bits(acc, f32(0.5, 2.25, 1e8, 0, 0.1, 0.2, np.float32(0.3) + np.float32(7), np.float32(0.4) + np.float32(8),
                              109, 200)) and same_bits(g, G)
    assert acc[2] == np.float32(1e8)                        # 1e8 + 3 rounds back to 1e8 in float32: f32 arithmetic
    acc, g = GO.accumulate(GO.CLOSE, ACC, G, ROWS, 0.5)
    assert same_bits(g, f32(1, 0.125, 5e7, -2, 5, 6, np.float32(0.3) * np.float32(0.5), np.float32(0.4) * np.float32(0.5),
                            50, 10)) and same_bits(acc, ACC)
    acc, g = GO.accumulate(GO.ADD_CLOSE, ACC, G, ROWS, 0.5)
    assert same_bits(g, f32(1, 1.125, 5e7, 0, 5, 6, (np.float32(0.3) + np.float32(7)) * np.float32(0.5),
                            (np.float32(0.4) + np.float32(8)) * np.float32(0.5), 54.5, 10)) and same_bits(acc, ACC)
    # the malformed rows (8, 12) and (-1, 2) wrote nothing: elements 0 and 9 keep their bits in every mode
    for mode in GO.MODES:
        acc, g = GO.accumulate(mode, ACC, G, ROWS, 0.25)
        assert same_bits(acc[[0, 9]], ACC[[0, 9]]) and same_bits(g[[0, 9]], G[[0, 9]])


def test_scale_is_rounded_to_float32_once_and_every_operation_rounds():
    third = np.float32(1.0 / 3.0)
    _, g = GO.accumulate(GO.ADD_CLOSE, f32(0.1, 0.1), f32(0.2, 0.7), [(0, 2)], 1.0 / 3.0)
    assert same_bits(g, [(np.float32(0.1) + np.float32(0.2)) * third, (np.float32(0.1) + np.float32(0.7)) * third])
    assert float(g[0]) != (0.1 + 0.2) / 3.0                 # not the double statement


def test_clip_cuts_a_row_mid_way():
    for mode in GO.MODES:
        full = GO.accumulate(mode, ACC, G, ROWS, 0.5)
        cut = GO.accumulate(mode, ACC, G, ROWS, 0.5, clip=(2, 8))
        for got, whole, old in zip(cut, full, (ACC, G)):
            assert same_bits(got[2:8], whole[2:8])                             # inside the clip: the launch's values
            assert same_bits(got[:2], old[:2]) and same_bits(got[8:], old[8:])   # rows (1, 4) and (6, 9) were cut
    # the clip is clamped to the buffer, an empty one touches nothing
    assert all(same_bits(a, b) for a, b in zip(GO.accumulate(GO.ADD, ACC, G, ROWS, clip=(-5, 99)),
                                               GO.accumulate(GO.ADD, ACC, G, ROWS)))
    for clip in ((5, 5), (7, 3)):
        acc, g = GO.accumulate(GO.ADD_CLOSE, ACC, G, ROWS, 0.5, clip=clip)
        assert same_bits(acc, ACC) and same_bits(g, G)


def test_scale_one_is_the_plain_sum():
    rs = np.random.RandomState(0)
    grads = [rs.randn(64).astype(np.float32) for _ in range(3)]
    rows = [(3, 40), (41, 64)]
    got = GO.accumulated_gradient(grads, rows, 1.0)
    want = grads[2].copy()
    for lo, hi in rows:
        want[lo:hi] = (grads[0][lo:hi] + grads[1][lo:hi]).astype(np.float32) + grads[2][lo:hi]
    assert same_bits(got, want)
    assert same_bits(GO.flushed_gradient(grads, rows, 1.0), want)              # open, add, add, close: the same sum
    assert same_bits(got[:3], grads[2][:3]) and same_bits(got[40:41], grads[2][40:41])


def test_open_over_nan_garbage():
    garbage = np.full(10, np.nan, dtype=np.float32)
    acc, g = GO.accumulate(GO.OPEN, garbage, G, [(0, 10)])
    assert same_bits(acc, G) and same_bits(g, G)
    acc, _ = GO.accumulate(GO.OPEN, garbage, G, [(2, 5)])
    assert same_bits(acc[2:5], G[2:5]) and np.isnan(acc[:2]).all() and np.isnan(acc[5:]).all()
    _, g = GO.accumulate(GO.ADD_CLOSE, acc, G, [(2, 5)], 0.5)                  # the garbage outside the rows stays there
    assert same_bits(g, f32(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)) and np.isfinite(g).all()


# ---------------------------------------------------------------- 2. the cycle schedule
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("batches", [5, 6])
def test_cycle_schedule(n, batches):
    events = GO.schedule(n, batches, n_epochs=2, loss_reduction="mean")
    per_epoch = len(events) // 2
    assert per_epoch == batches + (n > 1)
    updates = -(-batches // n)
    for e in range(2):
        ev = events[e * per_epoch:(e + 1) * per_epoch]
        assert [x[0] for x in ev] == ["step"] * batches + ["flush"] * (n > 1)
        assert ev[-1][4] == (e + 1) * updates and ev[-1][3] == 0               # no gradient crosses an epoch
        if n == 1:
            assert all(x[1] is None and x[2] is None for x in ev)
            assert [x[4] for x in ev] == [e * updates + i + 1 for i in range(batches)]
            continue
        for i, (event, launch, scale, pending, count) in enumerate(ev[:-1]):
            pos = i % n + 1
            assert launch == ("open" if pos == 1 else "add") if pos < n else launch == "add-close"
            assert scale == (1.0 / n if pos == n else None)
            assert pending == pos % n and count == e * updates + (i + 1) // n
        m = batches % n
        assert ev[-1][1:3] == (("close", 1.0 / m) if m else (None, None))
    table = {(2, 5): ["open", "add-close", "open", "add-close", "open", "close"],
             (3, 5): ["open", "add", "add-close", "open", "add", "close"],
             (3, 6): ["open", "add", "add-close", "open", "add", "add-close", None]}
    if (n, batches) in table:
        assert [x[1] for x in events[:per_epoch]] == table[(n, batches)]
    if (n, batches) == (3, 5):
        assert events[per_epoch - 1][2] == 0.5 and [x[4] for x in events[:per_epoch]] == [0, 0, 1, 1, 1, 2]
    assert all(x[2] in (None, 1.0) for x in GO.schedule(n, batches, loss_reduction="sum"))


# ---------------------------------------------------------------- 3. the entry point
def test_entry_point_is_exported_and_declared():
    protos = _lib.parse_header()
    assert "cova_grad_accumulate" in protos and hasattr(ctypes.CDLL(_lib.LIB_PATH), "cova_grad_accumulate")
    assert protos["cova_grad_accumulate"] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
                                              ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong,
                                              ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p]
    fn = _lib.lib().fn["cova_grad_accumulate"]
    # no rows or no elements: no launch, status 0 (needs no device); an unknown mode is an error
    assert fn(1, None, None, 0, None, 0, 0, 0, 0, 1.0, None) == 0
    assert fn(3, None, None, 16, None, 0, 16, 0, 16, 0.5, None) == 0
    assert fn(4, None, None, 16, None, 0, 16, 0, 16, 0.5, None) != 0
    assert fn(-1, None, None, 16, None, 0, 16, 0, 16, 0.5, None) != 0


# ---------------------------------------------------------------- 4. options and the default
@pytest.mark.parametrize("n", [0, -1, 2.5, "2", True, None])
def test_invalid_accumulate_steps_raise(n):
    with pytest.raises(ValueError, match="accumulate_steps"):
        trainer(accumulate_steps=n)


def test_default_adds_nothing():
    tr = trainer()
    assert tr.accumulate_steps == 1 and tr.accumulated == 0
    assert not any(hasattr(tr, n) for n in ("accbucket", "_acc_seg", "_acc_rows")) and tr._run_table.tensor is None
    assert set(tr.optimizer_state_dict()) == {"step", "exp_avg", "exp_avg_sq", "hp"}
    assert tr.flush() is False
    tr.step_count = 7
    assert tr.update_count == 7                             # one counter
    assert np.int64(3) == trainer(accumulate_steps=np.int64(3)).accumulate_steps


def test_table_holds_the_trainable_runs_only():
    tr = trainer(accumulate_steps=2, frozen=FROZEN)
    assert tr.accbucket.flat.numel() == tr.gbucket.flat.numel() and tr.accbucket.offsets == tr.gbucket.offsets
    seg = tr._acc_seg.tolist()
    lo_first = tr.pbucket.offsets["convnet.4.0.conv1.weight"][0]
    assert seg == [[lo_first, tr.pbucket.flat.numel(), 0, 0]] and tr._run_table.total == tr.pbucket.flat.numel() - lo_first
    assert all(tr.pbucket.offsets[k][0] + tr.pbucket.offsets[k][1] <= lo_first for k in tr.frozen)
    full = trainer(accumulate_steps=2)
    assert full._acc_seg.tolist() == [[0, full.pbucket.flat.numel(), 0, 0]]
    # a frozen tensor in the middle splits the runs; `start` is the running length
    mid = trainer(accumulate_steps=3, frozen=("bbox_feat_encoder.0.weight",))
    rows = mid._acc_seg.tolist()
    o, m, _ = mid.pbucket.offsets["bbox_feat_encoder.0.weight"]
    assert len(rows) == 2 and rows[0][:2] == [0, o] and rows[1][0] == (o + m + 3) // 4 * 4
    assert rows[1][3] == o and mid._run_table.total == sum(r[1] - r[0] for r in rows)


# ---------------------------------------------------------------- 5. the cycle, launches recorded instead of issued
@pytest.fixture
def launches(monkeypatch):
    calls = []
    monkeypatch.setattr(T.engine, "call", lambda name, *a: calls.append((name,) + a))
    return calls


def host_cycle(tr):
    """train_step() with forward_backward replaced by its host effect (the micro-batch counter)."""
    def forward_backward(batch, masks=None):
        tr.step_count += 1
        tr._head_work = None
        return None, None
    tr.forward_backward = forward_backward


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("n, batches", [(2, 5), (3, 5), (3, 6)])
def test_launches_and_counters_follow_the_schedule(launches, n, batches, reduction):
    tr = trainer(accumulate_steps=n, loss_reduction=reduction)
    host_cycle(tr)
    numel = tr.gbucket.flat.numel()
    steps = 0
    for event, launch, scale, pending, count in GO.schedule(n, batches, n_epochs=2, loss_reduction=reduction):
        del launches[:]
        if event == "step":
            tr.train_step({})
            steps += 1
        else:
            assert tr.flush() is (launch is not None)
        acc = [c for c in launches if c[0] == "cova_grad_accumulate"]
        adam = [c for c in launches if c[0] == "cova_adam_step"]
        assert (tr.accumulated, tr.update_count, tr.step_count) == (pending, count, steps)
        if launch is None:
            assert not launches
            continue
        assert len(acc) == 1 and launches[0] is acc[0]                         # one launch, before the update
        name, mode, a, g, nn, seg, n_seg, total, lo, hi, s = acc[0]
        assert GO.MODES[mode] == launch and a is tr.accbucket.flat and g is tr.gbucket.flat
        assert (nn, n_seg, total, lo, hi) == (numel, 1, numel, 0, numel) and seg is tr._acc_seg
        assert s == (1.0 if scale is None else scale)
        if launch in ("close", "add-close"):
            assert len(adam) == 1 and adam[0][6] == count                      # Adam's step is the update number
        else:
            assert not adam


def test_average_follows_the_updates(launches):
    tr = trainer(accumulate_steps=2, average="swa", average_start=2)
    host_cycle(tr)
    for _ in range(3):                                       # one update: before the start
        tr.train_step({})
    assert (tr.update_count, tr.n_averaged, tr.accumulated) == (1, 0, 1)
    tr.train_step({})                                        # update 2: the copy
    assert (tr.update_count, tr.n_averaged) == (2, 1)
    del launches[:]
    tr.train_step({})
    assert not [c for c in launches if c[0] == "cova_weight_average"]          # a micro-step: the average rests
    tr.train_step({})
    assert (tr.update_count, tr.n_averaged) == (3, 2)
    assert len([c for c in launches if c[0] == "cova_weight_average"]) == 2


# ---------------------------------------------------------------- 6. state
def test_state_dict_rules(launches):
    tr = trainer(accumulate_steps=3)
    host_cycle(tr)
    for _ in range(4):
        tr.train_step({})
    assert (tr.step_count, tr.update_count, tr.accumulated) == (4, 1, 1)
    for method in (tr.optimizer_state_dict, tr.optimizer_step, tr.broadcast_state):
        with pytest.raises(ValueError, match=r"train_step\(\).*flush\(\)"):   # mid-cycle
            method()
    assert tr.flush() is True
    st = tr.optimizer_state_dict()
    assert (st["step"], st["updates"]) == (4, 2)
    # into a trainer that does not accumulate: refused, naming the option
    plain = trainer()
    with pytest.raises(ValueError, match="accumulate_steps"):
        plain.load_optimizer_state_dict(st)
    assert plain.step_count == 0
    plain.load_optimizer_state_dict(dict(st, updates=4))     # (equal counters: nothing to lose)
    assert plain.step_count == plain.update_count == 4
    # into an accumulating trainer: both counters; pending micro-batches are dropped
    other = trainer(accumulate_steps=2)
    host_cycle(other)
    other.train_step({})
    assert other.accumulated == 1
    other.load_optimizer_state_dict(st)
    assert (other.step_count, other.update_count, other.accumulated) == (4, 2, 0)
    # a state without "updates" (written without accumulation): update_count = step
    old = {k: v for k, v in st.items() if k != "updates"}
    other.train_step({})
    other.load_optimizer_state_dict(old)
    assert (other.step_count, other.update_count, other.accumulated) == (4, 4, 0)
    other.train_step({})
    other.load_state_dict(SD)
    assert other.accumulated == 0 and other.flush() is False
    # a direct optimizer_step() at a cycle boundary is one update
    del launches[:]
    other.optimizer_step()
    assert other.update_count == 5 and [c[6] for c in launches if c[0] == "cova_adam_step"] == [5]


def test_flush_is_refused_inside_averaged_weights(launches):
    tr = trainer(accumulate_steps=2, average="ema")
    host_cycle(tr)
    tr.train_step({})
    with tr.averaged_weights():
        with pytest.raises(RuntimeError, match="averaged_weights"):
            tr.flush()
        with pytest.raises(RuntimeError, match="averaged_weights"):
            tr.train_step({})
    assert tr.accumulated == 1 and tr.flush() is True


# ---------------------------------------------------------------- 7. fit
class CountingTrainer:
    """The host surface fit() uses, with the accumulation counters kept as the schedule states them."""

    def __init__(self, n):
        self.cfg, self.device, self.param_groups = dict(n_classes=4), "cpu", [dict(lr=1.0)]
        self.metrics, self.accumulate_steps, self.accumulated, self.update_count, self.log = self, n, 0, 0, []

    def train_step(self, batch):
        self.accumulated += 1
        self.log.append(("step", self.param_groups[0]["lr"]))
        if self.accumulated == self.accumulate_steps:
            self.accumulated, self.update_count = 0, self.update_count + 1

    def flush(self):
        self.log.append(("flush", self.param_groups[0]["lr"]))
        if self.accumulated:
            self.accumulated, self.update_count = 0, self.update_count + 1

    def read(self):
        self.log.append(("read", getattr(self, "accumulated", 0)))
        conf = np.eye(4, dtype=np.int64)
        return dict(confusion=conf, kept=4, loss_numerator=4.0, loss_denominator=4.0)

    def reset(self):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, sd, broadcast=False):
        pass


class FiveBatches:
    def batches(self, batch_size, **kw):
        return iter([{}] * 5)


@pytest.mark.parametrize("n, updates", [(1, 5), (2, 3), (3, 2)])
def test_fit_flushes_at_the_end_of_every_epoch(monkeypatch, n, updates):
    tr = CountingTrainer(n)
    if n == 1:
        del tr.accumulate_steps, tr.update_count, tr.accumulated             # today's surface: neither is asked for
        tr.train_step = lambda batch: tr.log.append(("step", tr.param_groups[0]["lr"]))

    def scripted(trainer, dataset, **kw):
        tr.log.append(("eval", getattr(trainer, "accumulated", 0)))
        return evaluation.EvalReport(np.zeros((10, 3), dtype=np.int32))
    monkeypatch.setattr(evaluation, "evaluate_split", scripted)
    res = evaluation.fit(tr, FiveBatches(), None, 2, 5, eval_interval=1, lr_schedule=lambda epoch: 0.5 ** epoch)
    assert [h["updates"] for h in res.history] == [updates, updates]
    flush = [("flush", 1.0)] if n > 1 else []
    assert tr.log[:len(flush) + 7] == [("step", 1.0)] * 5 + flush + [("read", 0), ("eval", 0)]
    # the schedule applies after the flush: the second epoch's steps and flush see the new rate
    second = tr.log[len(flush) + 7:]
    assert second == [("step", 0.5)] * 5 + [(f, 0.5) for f, _ in flush] + [("read", 0), ("eval", 0)]


# ---------------------------------------------------------------- 8. two ranks
def _counter_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    # momentum flags and the average's counter travel in the same message as the two step counters
    tr = HotPathTrainer(CFG, SD, "cpu", world_size=world, accumulate_steps=2, optimizer="sgd", momentum=0.9,
                        average="ema")
    tr.step_count, tr._update_count, tr.n_averaged, tr._buf_exists = 20 + rank, 9 + rank, 4 + rank, [rank == 0]
    tr.broadcast_state(src=0)
    res["after"] = (tr.step_count, tr.update_count, tr.n_averaged, list(tr._buf_exists))
    tr.accumulated = 1                                       # mid-cycle: refused before any collective
    try:
        tr.broadcast_state(src=0)
        res["pending"] = None
    except ValueError as e:
        res["pending"] = str(e)
    tr.accumulated = 0
    st = dict(tr.optimizer_state_dict(), step=40 + rank, updates=15 + rank)
    tr.load_optimizer_state_dict(st, broadcast=True)
    res["loaded"] = (tr.step_count, tr.update_count, tr.accumulated)
    # a trainer that does not accumulate refuses rank 1's state with unequal counters, on both ranks
    plain = HotPathTrainer(CFG, SD, "cpu", world_size=world)
    st1 = dict(plain.optimizer_state_dict(), step=7, updates=7 if rank == 0 else 3)
    try:
        plain.load_optimizer_state_dict(st1, broadcast=True)
        res["raised"] = None
    except (KeyError, ValueError) as e:
        res["raised"] = type(e).__name__
    torch.save(res, os.path.join(out_dir, "c%d.pt" % rank))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_counters_travel_with_broadcast_state_and_a_broadcast_optimizer_state(tmp_path):
    world, port = 2, free_port()
    mp.spawn(_counter_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in (torch.load(os.path.join(str(tmp_path), "c%d.pt" % r)) for r in range(world)):
        assert r["after"] == (20, 9, 4, [True])              # rank 0's
        assert "flush()" in r["pending"]
        assert r["loaded"] == (40, 15, 0)
        assert r["raised"] is not None                       # on the rank that validated too
