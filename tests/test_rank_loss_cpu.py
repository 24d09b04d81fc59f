"""Host side of the per-page ranking loss (no GPU): tests/rank_oracle.py against torch autograd in float64 (logsumexp over
the masked rows, gradient from backward), the refusals of engine.check_rank_options / HotPathTrainer / CrossEntropyLoss,
what the defaults leave as before, and the declared entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.models import CrossEntropyLoss  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import rank_oracle as RO  # noqa: E402
from config_cases import BASE as CFG  # noqa: E402

SD = weights.seeded_state_dict(3, **{k: v for k, v in CFG.items() if k != "drop_prob"})
SIZES = [0, 1, 2, 65, 230]
HEAD, TAIL = 3, 4                                  # rows outside every page
TOL = 1e-12                                        # float64 against float64: |a - b| <= TOL * (1 + |b|)


def batch(nc, seed):
    """the issue's page sizes with outside rows; lists with 0, 1 and 2 targets, ignored and bad labels in between"""
    g = torch.Generator().manual_seed(seed)
    n = HEAD + sum(SIZES) + TAIL
    page_start = HEAD + np.concatenate([[0], np.cumsum(SIZES)])
    logits = torch.randn(n, nc, generator=g) * 4
    labels = torch.where(torch.rand(n, generator=g) < 0.9, torch.zeros(n, dtype=torch.int64),
                         torch.randint(1, nc, (n,), generator=g))
    labels[torch.rand(n, generator=g) < 0.05] = -100
    labels[torch.rand(n, generator=g) < 0.05] = nc + 3
    start = {sz: int(page_start[i]) for i, sz in enumerate(SIZES)}
    labels[start[1]] = 1                                                   # one candidate, its own target: L = 0
    labels[start[2]:start[2] + 2] = torch.tensor([0, -100])                # no target at all
    s = start[65]
    labels[s:s + 65][labels[s:s + 65] == 1] = 0
    labels[s + 7] = labels[s + 40] = 1                                     # two targets of class 1
    labels[s + 8], labels[s + 9] = -100, nc + 3
    labels[:HEAD] = 1                                                      # outside rows: no part, whatever they carry
    labels[n - TAIL:] = nc - 1
    return logits, labels, page_start, start


def torch_reference(logits, labels, page_start, w, ignore, weight, reduction):
    """the loss from torch.logsumexp over the masked rows in float64, the gradient from backward"""
    x = logits.double().clone().requires_grad_(True)
    n, nc = x.shape
    cand = (labels >= 0) & (labels < nc)
    if ignore is not None:
        cand &= labels != ignore
    num, den, L = x.new_zeros(()), 0.0, {}
    ps = [min(max(int(v), 0), n) for v in page_start]
    for p in range(len(ps) - 1):
        inside = torch.zeros(n, dtype=torch.bool)
        inside[ps[p]:max(ps[p + 1], ps[p])] = True
        for c in range(1, nc):
            rows, tgt = inside & cand, inside & cand & (labels == c)
            if not bool(tgt.any()):
                continue
            L[p, c] = torch.logsumexp(x[rows, c], 0) - torch.logsumexp(x[tgt, c], 0)
            wc = 1.0 if w is None else float(w[c])
            num, den = num + wc * L[p, c], den + wc
    R = num if reduction == "sum" else (num / den if den > 0 else num * 0.0)
    loss = weight * R
    if loss.requires_grad:
        loss.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return float(loss), {k: float(v) for k, v in L.items()}, grad.numpy(), den


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= TOL * (1 + np.abs(b))).all())


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("nc", [2, 4, 16])
def test_oracle_against_torch_autograd(nc, reduction):
    logits, labels, page_start, start = batch(nc, 40 + nc)
    w = None if nc == 2 else torch.linspace(0.5, 3.0, nc).double()
    for ignore in (None, -100, 1):                                         # 1: the targets of class 1 carry the ignore label
        out = RO.rank_loss(logits.numpy(), labels.numpy(), page_start, None if w is None else w.numpy(), ignore, 0.7,
                           reduction)
        loss, L, grad, den = torch_reference(logits, labels, page_start, w, ignore, 0.7, reduction)
        assert close(out["loss"], loss), (out["loss"], loss)
        assert sorted(L) == [(int(p), int(c) + 1) for p, c in zip(*np.nonzero(out["scored"]))]
        for (p, c), v in L.items():
            assert close(out["L"][p, c - 1], v), (p, c)
        assert close(out["dlogits"], grad)
        assert close(out["acc"][1], den) and out["acc"][2] == len(L)
        by_size = {sz: i for i, sz in enumerate(SIZES)}
        lists = out["lists"]
        assert not out["scored"][by_size[0]].any() and not lists[by_size[0]].any()
        assert not out["scored"][by_size[2]].any() and (lists[by_size[2], :, 2] == 1).all()
        if ignore == 1:
            assert not out["scored"][:, 0].any() and not out["target"][:, 1].any()
            assert (lists[by_size[1], :, 2] == 0).all()
        else:
            p = by_size[1]
            assert out["scored"][p, 0] and out["L"][p, 0] == 0.0 and not out["dlogits"][start[1]].any()
            assert lists[by_size[65], 0, 3] == 2
        n = labels.numel()
        assert not out["dlogits"][:HEAD].any() and not out["dlogits"][n - TAIL:].any() and not out["dlogits"][:, 0].any()
        assert not out["dlogits"][~out["cand"]].any()
        bad = (labels.numpy() == nc + 3) | (labels.numpy() == -100 if ignore == -100 else False)
        assert not out["cand"][bad].any()


def test_zero_denominator_and_grad_scale():
    logits, labels, page_start, _ = batch(4, 9)
    none = torch.where((labels >= 1) & (labels < 4), torch.zeros_like(labels), labels)     # no target anywhere
    for lab, w in ((none, None), (labels, np.zeros(4))):                                   # or every weight zero
        for reduction in ("sum", "mean"):
            out = RO.rank_loss(logits.numpy(), lab.numpy(), page_start, w, -100, 2.0, reduction)
            assert out["acc"][1] == 0.0 and out["loss"] == 0.0 and not out["dlogits"].any()
            loss, _, grad, _ = torch_reference(logits, lab, page_start, None if w is None else torch.tensor(w), -100,
                                               2.0, reduction)
            assert loss == 0.0 and not grad.any()
    a = RO.rank_loss(logits.numpy(), labels.numpy(), page_start, None, -100, 1.0, "mean")
    b = RO.rank_loss(logits.numpy(), labels.numpy(), page_start, None, -100, 1.0, "mean", grad_scale=0.25)
    assert a["loss"] == b["loss"] and np.array_equal(0.25 * a["dlogits"], b["dlogits"])
    # the mean is over the scored lists' weights
    s = RO.rank_loss(logits.numpy(), labels.numpy(), page_start, None, -100, 1.0, "sum")
    assert close(s["loss"] / s["acc"][1], a["loss"]) and s["acc"][1] == s["acc"][2] > 0


def test_check_rank_options():
    assert engine.check_rank_options(0) == 0.0 and engine.check_rank_options(0.5) == 0.5
    assert engine.check_rank_options(np.float32(1.5)) == 1.5 and engine.check_rank_options(np.int64(2)) == 2.0
    for bad in (-1, -0.5, float("nan"), float("inf"), "1", None, True, False):
        with pytest.raises(ValueError, match="page_rank_weight"):
            engine.check_rank_options(bad)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), "0.5", True, None])
def test_constructor_refusals(bad):
    with pytest.raises(ValueError, match="page_rank_weight"):
        HotPathTrainer(CFG, SD, "cpu", page_rank_weight=bad)
    with pytest.raises(ValueError, match="page_rank_weight"):
        CrossEntropyLoss(page_rank_weight=bad)


def test_trainer_options():
    plain = HotPathTrainer(CFG, SD, "cpu")
    assert plain._rank() == 0.0 and plain._criterion() is None and plain.loss_path == "cova_ce_sum"
    assert plain.loss_options == dict(label_smoothing=0.0, focal_gamma=0.0, ignore_index=None, loss_reduction="sum")
    assert plain.last_rank_lists is None and plain.last_rank_acc is None
    assert HotPathTrainer(CFG, SD, "cpu", page_rank_weight=0).loss_options == plain.loss_options
    tr = HotPathTrainer(CFG, SD, "cpu", page_rank_weight=0.5)
    assert tr._rank() == 0.5 and tr.loss_path == "cova_ce_loss" and tr._mining() is None
    assert tr._criterion() == dict(label_smoothing=0.0, focal_gamma=0.0, ignore_index=None, reduction="sum")
    assert tr.loss_options["page_rank_weight"] == 0.5
    assert set(tr.optimizer_state_dict()) == set(plain.optimizer_state_dict())
    # read and checked at every step, like the other scalar options
    tr.loss_options["page_rank_weight"] = 0.0
    assert tr._criterion() is None and tr.loss_path == "cova_ce_sum"
    tr.loss_options["page_rank_weight"] = -2.0
    with pytest.raises(ValueError, match="page_rank_weight"):
        tr._criterion()
    plain.loss_options["page_rank_weight"] = 1
    assert plain._rank() == 1.0 and plain.loss_path == "cova_ce_loss"
    # a batch without pages is refused before any launch, in the step and in the validation loss
    plain_batch = dict(bboxes=torch.zeros(3, 5), labels=torch.zeros(3, dtype=torch.int64))
    for fn in (plain.forward_backward, plain.loss):
        with pytest.raises(ValueError, match="page_start"):
            fn(plain_batch)


def test_module_options():
    m = CrossEntropyLoss()
    assert m.page_rank_weight == 0.0 and "page_rank" not in m.extra_repr()
    m = CrossEntropyLoss(page_rank_weight=0.7, weight=[1.0, 2.0, 3.0], reduction="sum")
    assert m.page_rank_weight == 0.7 and "page_rank_weight=0.7" in repr(m)
    with pytest.raises(ValueError, match="page_start"):
        m(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 3]))


def test_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    fwd, bwd = protos["cova_page_rank_loss_fwd"], protos["cova_page_rank_loss_bwd"]
    p, i, d, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    assert fwd == [p, p, p, i, i, i, p, ll, i, p, p, p]
    assert bwd == [p, p, p, i, i, i, p, ll, i, p, p, d, i, p, p, p, i, p]
    if os.path.exists(_lib.LIB_PATH):
        cdll = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(cdll, "cova_page_rank_loss_fwd") and hasattr(cdll, "cova_page_rank_loss_bwd")
