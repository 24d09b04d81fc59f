"""Host logic of HotPathTrainer's weight averaging (no GPU): the exported entry point, argument validation, what the
defaults leave exactly as before, the schedule, the table of the averaging launch, the state round trips, the view swap
of averaged_weights() and the broadcast of the average across two gloo ranks."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import cova_amd  # noqa: E402,F401  (spawned workers re-import this module without conftest.py)

import pytest  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

import average_oracle as AO  # noqa: E402
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


def host_step(tr):
    """What a step leaves for the averaging schedule, without device work: new parameters and statistics, the step
    count, then the end of optimizer_step() with the launch recorded instead of issued."""
    tr.step_count += 1
    for v in tr.params.values():                      # (the views: the alignment padding stays zero)
        v.add_(0.01 * tr.step_count)
    tr.buffers["convnet.1.running_mean"].add_(0.5)
    tr.buffers["convnet.1.num_batches_tracked"].add_(1)
    tr._average_step()


@pytest.fixture
def launches(monkeypatch):
    calls = []
    monkeypatch.setattr(T.engine, "call", lambda name, *a: calls.append((name,) + a))
    return calls


# ---------------------------------------------------------------- 1. the entry point
def test_entry_point_is_exported_and_declared():
    protos = _lib.parse_header()
    assert "cova_weight_average" in protos and hasattr(ctypes.CDLL(_lib.LIB_PATH), "cova_weight_average")
    assert protos["cova_weight_average"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p]
    # no rows or no elements: no launch, status 0 (needs no device)
    assert _lib.lib().fn["cova_weight_average"](None, None, 0, None, 0, 0, 0.5, None) == 0
    assert _lib.lib().fn["cova_weight_average"](None, None, 16, None, 0, 16, 0.5, None) == 0


# ---------------------------------------------------------------- 2. validation
@pytest.mark.parametrize("kw, match", [
    (dict(average="polyak"), "average must be"),
    (dict(average="ema", average_decay=1.0), "average_decay"),
    (dict(average="ema", average_decay=-0.1), "average_decay"),
    (dict(average="swa", average_decay=1.5), "average_decay"),
    (dict(average="ema", average_warmup=0), "average_warmup"),
    (dict(average="ema", average_warmup=2.5), "average_warmup"),
    (dict(average="swa", average_start=-1), "average_start"),
    (dict(average="swa", average_every=0), "average_every"),
    (dict(average_decay=0.99), "average_decay"),
    (dict(average_warmup=10), "average_warmup"),
    (dict(average_start=3), "average_start"),
    (dict(average_every=2), "average_every"),
    (dict(average_buffers=False), "average_buffers"),
])
def test_invalid_arguments_raise(kw, match):
    with pytest.raises(ValueError, match=match):
        trainer(**kw)


# ---------------------------------------------------------------- 3. off
def test_defaults_add_nothing():
    tr = trainer()
    assert tr.average is None and tr.n_averaged == 0
    assert set(tr.optimizer_state_dict()) == {"step", "exp_avg", "exp_avg_sq", "hp"}
    assert not any(hasattr(tr, n) for n in ("abucket", "abbucket", "bbucket", "tracked", "atracked", "_avg_seg"))
    assert not hasattr(tr, "_stat_table") and tr._run_table.tensor is None
    # the buffers are today's: separately allocated tensors
    ptrs = sorted((v.data_ptr(), v.numel() * v.element_size()) for v in tr.buffers.values())
    assert len({v.untyped_storage().data_ptr() for v in tr.buffers.values()}) == len(tr.buffers)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(ptrs, ptrs[1:]))
    for method in (tr.reset_average, tr.averaged_state_dict):
        with pytest.raises(RuntimeError, match="average="):
            method()
    with pytest.raises(RuntimeError, match="average="):
        with tr.averaged_weights():
            pass
    with pytest.raises(ValueError, match="average="):
        evaluation.fit(tr, None, None, 1, 1, use_average=True)


def test_averaging_trainer_keeps_keys_shapes_and_values():
    ref, tr = trainer(), trainer(average="ema")
    assert tr.average == T.AverageInfo("ema", 0.999, None, 0, 1, True, 1)            # start 0: begun at construction
    with pytest.raises(AttributeError):
        tr.average.n_averaged = 5                                                    # a read-only record
    a, b = ref.state_dict(), tr.state_dict()
    assert list(a) == list(b) and list(ref.buffers) == list(tr.buffers)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    avg = tr.averaged_state_dict()
    assert list(avg) == list(b) and all(torch.equal(avg[k], b[k]) and avg[k].shape == b[k].shape for k in b)
    # the float statistics are views of one flat buffer in state_dict order, live and averaged
    stats = [k for k in tr.buffers if not k.endswith("num_batches_tracked")]
    for bucket, views in ((tr.bbucket, tr.buffers), (tr.abbucket, tr._avg_buffers)):
        assert list(bucket.offsets) == stats
        for k, (o, m, _) in bucket.offsets.items():
            assert views[k].data_ptr() == bucket.flat.data_ptr() + 4 * o and views[k].numel() == m
    assert tr.abucket.offsets == tr.pbucket.offsets and tr.abucket.flat.data_ptr() != tr.pbucket.flat.data_ptr()
    nobuf = trainer(average="swa", average_buffers=False)
    assert nobuf._avg_buffers is nobuf.buffers and nobuf.abbucket is None
    assert nobuf.optimizer_state_dict()["average"]["buffers_flat"] is None


# ---------------------------------------------------------------- 4. the schedule
def test_schedule_function_values_and_the_warmup_crossover():
    f = T.average_weight
    assert [f("swa", 0.999, None, n) for n in (1, 2, 3, 9)] == [1 / 2, 1 / 3, 1 / 4, 1 / 10]
    assert f("swa", 0.5, 7, 3) == 1 / 4                                              # swa ignores decay and warmup
    assert f("ema", 0.999, None, 1) == f("ema", 0.999, None, 10 ** 6) == 1.0 - 0.999
    # warmup 10, decay 0.9: (1 + n) / (10 + n) < 0.9 while n < 80; equal at n = 80; the decay rules from there on
    assert f("ema", 0.9, 10, 1) == 1.0 - 2.0 / 11.0 and f("ema", 0.9, 10, 79) == 1.0 - 80.0 / 89.0
    assert f("ema", 0.9, 10, 79) > 1.0 - 0.9
    assert f("ema", 0.9, 10, 80) == f("ema", 0.9, 10, 81) == f("ema", 0.9, 10, 10 ** 9) == 1.0 - 0.9
    assert f("ema", 0.9, 1, 1) == 1.0 - 0.9                                          # warmup 1: (1 + n) / (1 + n) = 1
    for kind, decay, warmup in (("ema", 0.99, None), ("ema", 0.99, 5), ("swa", 0.999, None)):
        for n in range(1, 40):
            assert f(kind, decay, warmup, n) == AO.one_minus_decay(kind, decay, warmup, n)
            assert isinstance(f(kind, decay, warmup, n), float)


@pytest.mark.parametrize("kind, kw", [("ema", dict(average_warmup=3, average_decay=0.9)),
                                      ("swa", dict(average_start=2, average_every=2)),
                                      ("swa", dict(average_start=3, average_every=1, average_buffers=False)),
                                      ("ema", dict(average_start=1, average_every=3))])
def test_counter_and_launch_weights_follow_the_schedule(launches, kind, kw):
    tr = trainer(average=kind, **kw)
    a = tr.average
    assert a.n_averaged == (1 if a.start == 0 else 0)
    actions, n_end = AO.schedule(kind, a.decay, a.warmup, a.start, a.every, 9)
    p_at = {}
    for s, action in enumerate(actions, 1):
        del launches[:]
        host_step(tr)
        if action is None:
            assert launches == []
        elif action == "copy":
            assert launches == [] and torch.equal(tr.abucket.flat, tr.pbucket.flat) and tr.n_averaged == 1
            assert torch.equal(tr._avg_buffers["convnet.1.running_mean"], tr.buffers["convnet.1.running_mean"])
        else:
            assert [c[0] for c in launches] == ["cova_weight_average"] * (2 if a.buffers else 1)
            assert [c[-1] for c in launches] == [action] * len(launches)             # the double itself
            avg, p, n, seg, n_seg, total, _ = launches[0][1:]
            assert avg is tr.abucket.flat and p is tr.pbucket.flat and n == p.numel() == total and n_seg == 1
            assert seg is tr._avg_seg
            if a.buffers:
                avg, p, n, seg, n_seg, total, _ = launches[1][1:]
                assert avg is tr.abbucket.flat and p is tr.bbucket.flat and seg.tolist() == [[0, n, 0, 0]]
                assert (n, n_seg, total) == (p.numel(), 1, p.numel())
                assert torch.equal(tr.atracked, tr.tracked) and int(tr.atracked[0]) == s   # copied, not averaged
        p_at[s] = tr.n_averaged
    assert tr.average.n_averaged == n_end
    if kind == "swa" and kw.get("average_start") == 2:
        assert [p_at[s] for s in range(1, 10)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    tr.reset_average()
    assert tr.n_averaged == 1 and torch.equal(tr.abucket.flat, tr.pbucket.flat)
    late = trainer(average=kind, average_start=4)
    late.reset_average()
    assert late.n_averaged == 0                                                       # step 0 < start


# ---------------------------------------------------------------- 5. the table
def test_table_holds_the_trainable_runs_only():
    tr = trainer(average="swa", frozen=FROZEN, optimizer="adamw", param_groups=[{"params": "decoder.", "lr": 1e-3}])
    rows = tr._avg_seg.tolist()
    assert tr.frozen and len(rows) == len(tr._run_table.rows) >= 1
    start = 0
    for lo, hi, g, st in rows:
        assert 0 <= lo < hi <= tr.pbucket.flat.numel() and g == 0 and st == start
        start += hi - lo
    assert start == tr._run_table.total
    covered = torch.zeros(tr.pbucket.flat.numel(), dtype=torch.bool)
    for lo, hi, _, _ in rows:
        assert not covered[lo:hi].any()
        covered[lo:hi] = True
    for k, (o, m, _) in tr.pbucket.offsets.items():
        assert bool(covered[o:o + m].all()) == (k not in tr.frozen) and bool(covered[o:o + m].any()) == (k not in tr.frozen), k
    # group boundaries do not split the rows: the same runs as the optimizer's, merged across groups
    merged = []
    for lo, hi, _ in tr.optim_runs:
        if merged and merged[-1][1] == lo:
            merged[-1][1] = hi
        else:
            merged.append([lo, hi])
    assert [r[:2] for r in rows] == merged
    everything = trainer(average="ema", frozen=tuple(trainer().params))
    assert everything._avg_seg.shape == (0, 4) and everything._run_table.total == 0


# ---------------------------------------------------------------- 6. state round trips
def test_optimizer_state_carries_the_average(launches):
    tr = trainer(average="ema", average_decay=0.9, average_warmup=4)
    for _ in range(3):
        host_step(tr)
    tr.abucket.flat.uniform_()                                     # (the recorded launches wrote nothing)
    tr.abbucket.flat.uniform_()
    st = tr.optimizer_state_dict()
    assert set(st) == {"step", "exp_avg", "exp_avg_sq", "hp", "average"}
    avg = st["average"]
    assert (avg["kind"], avg["decay"], avg["warmup"], avg["start"], avg["every"], avg["buffers"], avg["n_averaged"]) == \
        ("ema", 0.9, 4, 0, 1, True, 4)
    assert avg["flat"].data_ptr() != tr.abucket.flat.data_ptr() and torch.equal(avg["flat"], tr.abucket.flat)
    # the documented resume: state dict first (the average restarts from it), then the optimizer state
    tr2 = trainer(weights.seeded_state_dict(5, **WCFG), average="ema", average_decay=0.9, average_warmup=4)
    tr2.load_state_dict(tr.state_dict())
    assert tr2.n_averaged == 1 and torch.equal(tr2.abucket.flat, tr.pbucket.flat)
    assert torch.equal(tr2.abbucket.flat, tr.bbucket.flat) and torch.equal(tr2.atracked, tr.tracked)
    tr2.load_optimizer_state_dict(st)
    assert tr2.step_count == 3 and tr2.n_averaged == 4
    assert torch.equal(tr2.abucket.flat, tr.abucket.flat) and torch.equal(tr2.abbucket.flat, tr.abbucket.flat)
    assert torch.equal(tr2.atracked, tr.atracked)
    a, b = tr.averaged_state_dict(), tr2.averaged_state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    # an absent key keeps the average load_state_dict left
    tr3 = trainer(average="ema")
    tr3.load_state_dict(tr.state_dict())
    tr3.load_optimizer_state_dict({k: v for k, v in st.items() if k != "average"})
    assert tr3.step_count == 3 and tr3.n_averaged == 1 and torch.equal(tr3.abucket.flat, tr.pbucket.flat)
    # another kind or size raises; a trainer without averaging takes the rest of the state
    with pytest.raises(ValueError, match="kind"):
        trainer(average="swa").load_optimizer_state_dict(st)
    for key in ("flat", "buffers_flat", "num_batches_tracked"):
        bad = dict(st, average=dict(avg, **{key: avg[key][:-1].clone()}))
        with pytest.raises(ValueError, match="wrong size"):
            trainer(average="ema").load_optimizer_state_dict(bad)
    with pytest.raises(ValueError, match="wrong size"):
        trainer(average="ema").load_optimizer_state_dict(dict(st, average=dict(avg, buffers_flat=None)))
    untouched = trainer(average="ema")
    with pytest.raises(ValueError):
        untouched.load_optimizer_state_dict(dict(st, average=dict(avg, flat=avg["flat"][:-4].clone())))
    assert untouched.step_count == 0 and untouched.n_averaged == 1               # validated before anything is copied
    plain = trainer()
    plain.load_optimizer_state_dict(st)
    assert plain.step_count == 3 and plain.average is None
    nobuf = trainer(average="ema", average_buffers=False)                         # its buffers are the live ones
    nobuf.load_optimizer_state_dict(st)
    assert nobuf.n_averaged == 4 and torch.equal(nobuf.abucket.flat, tr.abucket.flat)


# ---------------------------------------------------------------- 7. the view swap
@pytest.mark.parametrize("buffers", [True, False])
def test_averaged_weights_swaps_and_restores_the_views(buffers):
    tr = trainer(average="swa", average_buffers=buffers)
    tr.abucket.flat.add_(1.0)
    live_p, live_b = tr.params, tr.buffers
    key = "decoder.0.weight" if "decoder.0.weight" in tr.params else next(iter(tr.params))
    with tr.averaged_weights() as inside:
        assert inside is tr and tr.params is tr.abucket.views and tr.params is not live_p
        assert (tr.buffers is live_b) == (not buffers) and list(tr.buffers) == list(live_b)
        assert torch.equal(tr.params[key], live_p[key] + 1.0)
        assert all(torch.equal(v, tr.averaged_state_dict()[k]) for k, v in tr.state_dict().items())
        for call in (lambda: tr.train_step({}), lambda: tr.forward_backward({}), tr.optimizer_step,
                     lambda: tr.load_state_dict(SD), tr.reset_average):
            with pytest.raises(RuntimeError, match="averaged_weights"):
                call()
        with pytest.raises(RuntimeError, match="averaged_weights"):
            with tr.averaged_weights():
                pass
        assert tr.params is tr.abucket.views                                       # the refused calls changed nothing
    assert tr.params is live_p and tr.buffers is live_b and tr.step_count == 0
    with pytest.raises(KeyError):
        with tr.averaged_weights():
            raise KeyError("inside")
    assert tr.params is live_p and tr.buffers is live_b and not tr._avg_active
    late = trainer(average="swa", average_start=2)
    with pytest.raises(RuntimeError, match="not started"):
        with late.averaged_weights():
            pass
    with pytest.raises(RuntimeError, match="not started"):
        late.averaged_state_dict()
    assert late.params is late.pbucket.views


# ---------------------------------------------------------------- 8. two ranks
def _broadcast_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    tr = HotPathTrainer(CFG, weights.seeded_state_dict(40 + rank, **WCFG), "cpu", world_size=world, average="ema",
                        average_start=2)
    res["start"] = (tr.n_averaged, tr.pbucket.flat.clone())
    # rank-local averages and counters, then rank 0's everywhere
    tr.abucket.flat.fill_(1.0 + rank)
    tr.abbucket.flat.fill_(3.0 + rank)
    tr.atracked.fill_(5 + rank)
    tr.n_averaged, tr.step_count = 7 + 10 * rank, 20 + rank
    tr.broadcast_state(src=0)
    res["after"] = (tr.n_averaged, tr.step_count, tr.abucket.flat.clone(), tr.abbucket.flat.clone(), tr.atracked.clone())
    # a broadcast optimizer state carries rank 0's average too; one rank's bad average raises on both
    st = tr.optimizer_state_dict()
    st["average"]["flat"] = torch.full_like(st["average"]["flat"], 10.0 + rank)
    st["average"]["n_averaged"] = 30 + rank
    tr.load_optimizer_state_dict(st, broadcast=True)
    res["loaded"] = (tr.n_averaged, float(tr.abucket.flat[0]), float(tr.abucket.flat[-1]))
    bad = dict(st, average=dict(st["average"], kind="swa")) if rank == 1 else st
    try:
        tr.load_optimizer_state_dict(bad, broadcast=True)
        res["raised"] = None
    except (KeyError, ValueError) as e:
        res["raised"] = type(e).__name__
    # a broadcast state dict restarts the average from rank 0's weights on every rank
    tr.load_state_dict(weights.seeded_state_dict(50 + rank, **WCFG), broadcast=True)
    res["reloaded"] = (tr.n_averaged, torch.equal(tr.abucket.flat, tr.pbucket.flat), tr.pbucket.flat.clone())
    torch.save(res, os.path.join(out_dir, "a%d.pt" % rank))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_broadcast_state_sends_the_average_and_its_counter(tmp_path):
    world, port = 2, free_port()
    mp.spawn(_broadcast_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "a%d.pt" % r)) for r in range(world))
    assert r0["start"][0] == r1["start"][0] == 0 and torch.equal(r0["start"][1], r1["start"][1])
    for r in (r0, r1):
        n, step, flat, bflat, tracked = r["after"]
        assert (n, step) == (7, 20)
        assert bool((flat == 1.0).all()) and bool((bflat == 3.0).all()) and bool((tracked == 5).all())
        assert r["loaded"] == (30, 10.0, 10.0)
        assert r["raised"] is not None                                              # on the rank that validated too
        assert r["reloaded"][:2] == (1, True)
    assert torch.equal(r0["reloaded"][2], r1["reloaded"][2])
