"""Per-page hard-negative mining on the GPU: cova_hard_negative_select through the C ABI against tests/mining_oracle.py
(exact selection given the kernel's own scores, scores against float64, selection against the float64 oracle on decisive
inputs, reproducibility and page independence, refusals), HotPathTrainer with the option (launches, no host
synchronisation, wiring bit for bit against a trainer that is handed the mined labels) and the drop-in CrossEntropyLoss."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import cova_amd  # noqa: E402,F401

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from cova_web_object_detection_amd import _lib, engine  # noqa: E402
from cova_web_object_detection_amd.models import CrossEntropyLoss  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import mining_oracle as MO  # noqa: E402
from config_cases import TRAINER_CFG as CFG  # noqa: E402
from helpers import DEV, profiled  # noqa: E402
from trainer_cases import dev_batch, trainer_setup  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SELECT = "cova_hard_negative_select"
PAIR = ("cova_ce_loss_fwd", "cova_ce_loss_bwd")
SIZES = [0, 1, 2, 11, 64, 65, 230, 257, 1025, 3000]          # 3000: more than one LDS tile of the kernel
HEAD, TAIL = 5, 7                                             # rows before page_start[0] and from page_start[B] on


def run(logits, labels, page_start, ratio, min_keep, drop, scores=True, counts=True):
    """the entry point on device copies -> numpy (labels_out, scores, counts)"""
    out = engine.hard_negative_select(logits.to(DEV), labels.to(DEV), torch.as_tensor(page_start, dtype=torch.int64).to(DEV),
                                      ratio, min_keep, drop, want_scores=scores, want_counts=counts)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def mixed_batch(nc, seed):
    """the issue's page sizes in one batch with rows outside the pages, every label and logit pattern"""
    g = torch.Generator().manual_seed(seed)
    n = HEAD + sum(SIZES) + TAIL
    page_start = HEAD + np.concatenate([[0], np.cumsum(SIZES)])
    logits = torch.randn(n, nc, generator=g) * 4
    labels = torch.where(torch.rand(n, generator=g) < 0.9, torch.zeros(n, dtype=torch.int64),
                         torch.randint(1, nc, (n,), generator=g))
    labels[torch.rand(n, generator=g) < 0.04] = -100                       # interleaved: neither positive nor background
    labels[torch.rand(n, generator=g) < 0.04] = nc + 3
    start = {sz: int(page_start[i]) for i, sz in enumerate(SIZES)}
    labels[start[11]:start[11] + 11] = 0                                   # no positive: the quota is min_keep
    labels[start[64]:start[64] + 64] = nc - 1                              # no background
    labels[start[65]:start[65] + 65] = 1                                   # 60 positives, 5 background: quota >= n_bg
    labels[start[65] + 3:start[65] + 65:13] = 0
    for sz, step in ((230, 3), (257, 2), (1025, 5), (3000, 7)):            # duplicated logit rows: equal keys
        s = start[sz]
        logits[s + 1:s + sz:step] = logits[s]
    for sz in (230, 3000):
        s = start[sz]
        logits[s + 8, 0] = float("-inf")                                   # score +inf
        logits[s + sz - 2, nc - 1] = float("nan")                          # score NaN: ranks first
        labels[s + 8] = labels[s + sz - 2] = 0
    labels[:HEAD] = torch.tensor([0, 1, 0, -100, 0])                       # outside rows keep whatever they carry
    labels[n - TAIL:] = 0
    return logits, labels, page_start, start


# ------------------------------------------------------------------------------- 1. exact given the kernel's scores
@pytest.mark.parametrize("ratio, min_keep", [(3, 2), (0, 0), (0.5, 1), (40, 0)])
@pytest.mark.parametrize("nc", [2, 4, 16])
def test_selection_is_exact_given_the_kernels_scores(nc, ratio, min_keep):
    logits, labels, page_start, start = mixed_batch(nc, 100 + nc)
    drop = -100 if ratio == 0.5 else engine.MINED_OUT
    out, scores, counts = run(logits, labels, page_start, ratio, min_keep, drop)
    want, want_counts = MO.select_from_scores(scores, labels.numpy(), page_start, nc, ratio, min_keep, drop)
    assert np.array_equal(counts, want_counts), (counts.tolist(), want_counts.tolist())
    assert np.array_equal(out, want), np.nonzero(out != want)[0][:10]
    lab = labels.numpy()
    n = lab.shape[0]
    assert np.array_equal(out[:HEAD], lab[:HEAD]) and np.array_equal(out[n - TAIL:], lab[n - TAIL:])
    assert np.array_equal(out[lab != 0], lab[lab != 0])                    # only background rows are ever relabelled
    by_size = {sz: counts[i] for i, sz in enumerate(SIZES)}
    assert by_size[11].tolist() == [0, 11, min(min_keep, 11)] and by_size[64].tolist() == [64, 0, 0]
    assert by_size[65][1] == 5 and by_size[65][2] == (5 if ratio >= 0.5 else min_keep)
    assert by_size[0].tolist() == [0, 0, 0]
    for sz in (230, 3000):
        inf_row, nan_row = start[sz] + 8, start[sz] + sz - 2
        assert np.isnan(scores[nan_row]) and np.isposinf(scores[inf_row])
        if by_size[sz][2] >= 2:                                            # NaN first, +inf second: both kept
            assert out[nan_row] == 0 and out[inf_row] == 0
    if ratio == 0 and min_keep == 0:
        inside = np.zeros(n, dtype=bool)
        inside[HEAD:n - TAIL] = True
        assert (out[inside & (lab == 0)] == drop).all() and (counts[:, 2] == 0).all()
    # without the optional outputs the labels are the same
    only, none_s, none_c = run(logits, labels, page_start, ratio, min_keep, drop, scores=False, counts=False)
    assert none_s is None and none_c is None and np.array_equal(only, out)


def test_single_page_batch():
    g = torch.Generator().manual_seed(7)
    n, nc = 300, 4
    logits = torch.randn(n, nc, generator=g) * 4
    labels = torch.where(torch.rand(n, generator=g) < 0.95, torch.zeros(n, dtype=torch.int64),
                         torch.randint(1, nc, (n,), generator=g))
    for page_start in ([0, n], [10, 280], [-5, n + 9]):                    # the last: clamped to [0, N]
        out, scores, counts = run(logits, labels, page_start, 3, 2, -100)
        want, want_counts = MO.select_from_scores(scores, labels.numpy(), page_start, nc, 3, 2, -100)
        assert np.array_equal(out, want) and np.array_equal(counts, want_counts)
        assert 0 < counts[0, 2] < counts[0, 1]


# --------------------------------------------------------------------------------------- 2. scores against float64
@pytest.mark.parametrize("nc", [2, 4, 16])
def test_scores_against_float64(nc):
    # The gate counts f32 operations, it is not measured: NC expf and NC - 1 additions (terms <= 1, sum <= NC), the
    # roundings of l - m inside expf's argument, logf, m + log (one rounding at |lse|) and lse - l[0] (one at |s|), with
    # a factor 2 for the library functions: |error| <= 2 eps (NC + 4 + |lse| + |s|).
    g = torch.Generator().manual_seed(20 + nc)
    n = 5000
    logits = torch.randn(n, nc, generator=g) * 4
    labels = torch.zeros(n, dtype=torch.int64)
    _, scores, _ = run(logits, labels, [0, 2500, n], 1, 0, -100, counts=False)
    s64, lse64 = MO.scores64(logits.numpy())
    err = np.abs(scores.astype(np.float64) - s64)
    gate = 2 * EPS32 * (nc + 4 + np.abs(lse64) + np.abs(s64))
    print("NC %d: max |score - s64| %.3e, max error / gate %.3f" % (nc, err.max(), (err / gate).max()))
    assert (err <= gate).all(), (err / gate).max()


# ------------------------------------------------------------------- 3. against the float64 oracle, decisive inputs
def decisive_batch(seed, nc=4):
    """randn * 4 logits, 97 % background, 24 pages of 11..230 rows"""
    rs = np.random.RandomState(seed)
    sizes = rs.randint(11, 231, 24)
    sizes[:2] = (11, 230)
    n = int(sizes.sum())
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, nc, generator=g) * 4
    labels = torch.where(torch.rand(n, generator=g) < 0.97, torch.zeros(n, dtype=torch.int64),
                         torch.randint(1, nc, (n,), generator=g))
    return logits, labels, np.concatenate([[0], np.cumsum(sizes)])


@pytest.mark.parametrize("seed", [1, 4, 8])
def test_selection_equals_the_float64_oracle_on_decisive_inputs(seed):
    logits, labels, page_start = decisive_batch(seed)
    want, want_counts, gap, edge = MO.select(logits.numpy(), labels.numpy(), page_start, 3, 2, -100)
    # precondition on the inputs (checked with the CPU oracle when the seeds were chosen): no page's quota cuts between
    # two scores that f32 could order differently
    assert (gap >= 1e-4 * (1 + edge)).all(), (gap / (1 + edge)).min()
    assert ((want_counts[:, 2] > 0) & (want_counts[:, 2] < want_counts[:, 1])).all()      # every page is cut somewhere
    out, _, counts = run(logits, labels, page_start, 3, 2, -100, scores=False)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(out, want), np.nonzero(out != want)[0][:10]


# ---------------------------------------------------------------------- 4. reproducibility and page independence
def test_reproducible_and_independent_of_the_batch_around_a_page():
    g = torch.Generator().manual_seed(31)
    sizes, nc = [0, 1, 17, 230, 300, 2500], 4
    n = sum(sizes)
    page_start = np.concatenate([[0], np.cumsum(sizes)])
    logits = torch.randn(n, nc, generator=g) * 4
    logits[5::3] = logits[4]                                               # ties in every page
    labels = torch.where(torch.rand(n, generator=g) < 0.95, torch.zeros(n, dtype=torch.int64),
                         torch.randint(1, nc, (n,), generator=g))
    first = run(logits, labels, page_start, 3, 2, -100)
    again = run(logits, labels, page_start, 3, 2, -100)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (first[0] == -100).any()

    def part(lo, hi):                                                      # pages lo .. hi-1 as a batch of their own
        r0, r1 = int(page_start[lo]), int(page_start[hi])
        if r1 == r0:                                                       # N >= 1: an empty page has nothing to compare
            return
        out = run(logits[r0:r1], labels[r0:r1], page_start[lo:hi + 1] - r0, 3, 2, -100)
        assert np.array_equal(out[0], first[0][r0:r1]), (lo, hi)
        assert np.array_equal(out[1].view(np.uint32), first[1][r0:r1].view(np.uint32)), (lo, hi)
        assert np.array_equal(out[2], first[2][lo:hi]), (lo, hi)

    for p in range(len(sizes)):
        part(p, p + 1)
    part(0, 3)
    part(3, len(sizes))


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_null_pointers_and_too_many_classes_are_refused():
    lg, lb = torch.zeros(8, 4, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    ps, out = torch.tensor([0, 8], device=DEV), torch.empty(8, dtype=torch.int64, device=DEV)

    def call(logits=lg, labels=lb, page_start=ps, B=1, N=8, NC=4, ratio=3.0, min_keep=0, labels_out=out):
        engine.call(SELECT, logits, labels, page_start, B, N, NC, ratio, min_keep, -100, labels_out, None, None)

    call()
    for kw in (dict(logits=None), dict(labels=None), dict(page_start=None), dict(labels_out=None), dict(NC=17), dict(NC=1),
               dict(B=0), dict(N=0), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio=float("inf")),
               dict(min_keep=-1)):
        with pytest.raises(_lib.CovaHipError, match="10001"):
            call(**kw)
    with pytest.raises(_lib.CovaHipError, match="10001"):
        engine.hard_negative_select(torch.zeros(8, 17, device=DEV), lb, ps, 3.0, 0, -100)


# ----------------------------------------------------------------------------------------------------- the trainer
def paged(batch, counts):
    """a device batch that carries page_start, as DeviceCollate / DeviceDataset batches do"""
    b = dev_batch(batch)
    b["page_start"] = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=DEV)
    return b


def page_counts(i):
    return [20 + 3 * i, 11 + 2 * i]                                         # trainer_setup's boxes_per_page


def test_trainer_launches():
    sd, batches = trainer_setup()
    tr = HotPathTrainer(CFG, sd, DEV, hard_negative_ratio=3, hard_negative_min=2)
    for b in (paged(batches[0], page_counts(0)), dev_batch(batches[1])):
        prof = profiled(lambda: tr.forward_backward(b))[1]
        assert prof.get(SELECT) == 1 and [prof.get(n) for n in PAIR] == [1, 1] and "cova_ce_sum" not in prof, prof
    ref = HotPathTrainer(CFG, sd, DEV)
    prof = profiled(lambda: ref.forward_backward(dev_batch(batches[0])))[1]
    assert prof.get("cova_ce_sum") == 1 and SELECT not in prof and not any(n in prof for n in PAIR), prof
    # mining is the only difference between the two profiles
    mined = profiled(lambda: tr.forward_backward(dev_batch(batches[0])))[1]
    for name in (SELECT,) + PAIR:
        mined.pop(name)
    prof.pop("cova_ce_sum")
    assert mined == prof


def test_train_step_with_mining_makes_no_host_synchronisation():
    sd, batches = trainer_setup()
    tr = HotPathTrainer(CFG, sd, DEV, hard_negative_ratio=3, hard_negative_min=2)
    with_ps, without = paged(batches[1], page_counts(1)), dev_batch(batches[2])
    assert "page_start" not in without
    tr.train_step(dev_batch(batches[0]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in (with_ps, without):
            loss, pred = tr.train_step(b)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert loss.is_cuda and pred.shape == without["labels"].shape
    assert tr.last_mined_labels.is_cuda and tr.last_mined_labels.dtype == torch.int64
    assert tr.last_mining_counts.is_cuda and tr.last_mining_counts.dtype == torch.int32
    assert tr.last_mining_counts.shape == (2, 3) and bool(torch.isfinite(loss).all())
    with pytest.raises(ValueError, match="page_start"):
        tr.forward_backward({k: v for k, v in without.items() if k != "images"})


def test_derived_page_start_equals_the_batchs():
    sd, batches = trainer_setup()
    a = HotPathTrainer(CFG, sd, DEV, hard_negative_ratio=3, hard_negative_min=2)
    b = HotPathTrainer(CFG, sd, DEV, hard_negative_ratio=3, hard_negative_min=2)
    a.forward_backward(paged(batches[0], page_counts(0)))
    b.forward_backward(dev_batch(batches[0]))
    assert torch.equal(a.last_mined_labels, b.last_mined_labels)
    assert torch.equal(a.last_mining_counts, b.last_mining_counts)
    assert int(a.last_mining_counts[:, :2].sum()) == batches[0]["labels"].numel()
    assert torch.equal(a.gbucket.flat, b.gbucket.flat)


@pytest.mark.parametrize("kw", [dict(), dict(loss_reduction="mean", class_weight=[1.0, 4.0, 2.0, 3.0])],
                         ids=["sum", "mean_weights"])
def test_trainer_wiring_bit_for_bit(kw):
    sd, batches = trainer_setup()
    a = HotPathTrainer(CFG, sd, DEV, hard_negative_ratio=3, hard_negative_min=2, **kw)
    b = HotPathTrainer(CFG, sd, DEV, ignore_index=-100, **kw)
    plain = HotPathTrainer(CFG, sd, DEV, **kw)
    # validation does not mine: every row is scored (before any step: the three trainers hold the same state)
    first = dev_batch(batches[0])
    assert torch.equal(a.loss(first).view(torch.int32), plain.loss(first).view(torch.int32))
    for i in range(2):
        batch = dev_batch(batches[i])
        loss_a, pred_a = a.forward_backward(batch)
        mined = a.last_mined_labels
        assert mined.shape == batch["labels"].shape and pred_a.shape == batch["labels"].shape
        dropped = mined == engine.MINED_OUT
        assert bool(dropped.any()) and bool((batch["labels"][dropped] == 0).all())
        assert torch.equal(mined[~dropped], batch["labels"][~dropped])
        relabelled = torch.where(dropped, torch.full_like(mined, -100), mined)
        loss_b, pred_b = b.forward_backward(dict(batch, labels=relabelled))
        assert torch.equal(loss_a.view(torch.int32), loss_b.view(torch.int32)), (loss_a.item(), loss_b.item())
        assert torch.equal(pred_a, pred_b)
        assert torch.equal(a.gbucket.flat.view(torch.int32), b.gbucket.flat.view(torch.int32))
        counts = a.last_mining_counts.cpu()
        assert counts.shape == (2, 3) and counts[:, :2].sum(dim=1).tolist() == page_counts(i)
        for n_pos, n_bg, k in counts.tolist():
            assert k <= max(2, 3 * n_pos) and k == min(n_bg, max(2, 3 * n_pos))
        assert int(dropped.sum()) == int((counts[:, 1] - counts[:, 2]).sum())
        a.optimizer_step(), b.optimizer_step()
        assert torch.equal(a.pbucket.flat, b.pbucket.flat)


def test_trainer_with_its_own_ignore_label_drops_to_it():
    sd, batches = trainer_setup()
    tr = HotPathTrainer(CFG, sd, DEV, ignore_index=-100, hard_negative_ratio=0, hard_negative_min=1, track_metrics=True)
    batch = dev_batch(batches[0])
    batch["labels"] = batch["labels"].clone()
    batch["labels"][3::7] = -100
    tr.forward_backward(batch)
    mined, counts = tr.last_mined_labels.cpu(), tr.last_mining_counts.cpu()
    assert counts[:, 2].tolist() == [1, 1] and not bool((mined == engine.MINED_OUT).any())
    assert int((mined == 0).sum()) == 2
    # metrics count the scored rows: the positives and one background row a page
    out = tr.metrics.read()
    assert out["kept"] == int(counts[:, 0].sum()) + 2 and out["bad_labels"] == 0


# ------------------------------------------------------------------------------------------------------ the module
def test_module_equals_the_c_abi_path():
    logits, labels, page_start = decisive_batch(5)
    lg, lb = logits.to(DEV), labels.to(DEV)
    ps = torch.as_tensor(page_start, dtype=torch.int64, device=DEV)
    w = torch.tensor([1.0, 3.0, 2.0, 4.0])
    for kw in (dict(), dict(weight=w, reduction="sum", label_smoothing=0.1), dict(ignore_index=-1)):
        crit = CrossEntropyLoss(hard_negative_ratio=3, hard_negative_min=2, **kw).to(DEV)
        x = lg.clone().requires_grad_(True)
        loss = crit(x, lb, ps)
        loss.backward()
        drop = kw.get("ignore_index", -100)
        mined, _, _ = engine.hard_negative_select(lg, lb, ps, 3, 2, drop)
        opts = dict(label_smoothing=kw.get("label_smoothing", 0.0), focal_gamma=0.0, ignore_index=drop,
                    reduction=kw.get("reduction", "mean"))
        wd = None if "weight" not in kw else w.to(DEV)
        acc, _ = engine.ce_loss_fwd(lg, mined, wd, opts, want_pred=False)
        one = torch.ones(1, device=DEV)
        want_loss, want_dl = engine.ce_loss_bwd(lg, mined, wd, opts, acc, grad_scale=one)
        assert torch.equal(loss.detach().view(torch.int32), want_loss[0].view(torch.int32))
        assert torch.equal(x.grad.view(torch.int32), want_dl.view(torch.int32))
        dropped = mined != lb
        assert bool(dropped.any()) and bool((mined[dropped] == drop).all()) and bool((lb[dropped] == 0).all())
        assert not bool(x.grad[dropped].any())                             # zero rows exactly where labels were dropped
        assert bool(x.grad[~dropped].abs().sum(dim=1).gt(0).all())
        with pytest.raises(ValueError, match="page_start"):
            crit(lg, lb)
        # without the ratio the module is today's: page_start or not, the labels go to the criterion as they are
        today = CrossEntropyLoss(**kw).to(DEV)
        acc0, _ = engine.ce_loss_fwd(lg, lb, wd, opts, want_pred=False)
        loss0, _ = engine.ce_loss_bwd(lg, lb, wd, opts, acc0, want_grad=False)
        assert torch.equal(today(lg, lb).view(torch.int32), loss0[0].view(torch.int32))
        assert torch.equal(today(lg, lb, ps).view(torch.int32), loss0[0].view(torch.int32))
