#!/usr/bin/env python3
"""Generate tests/golden/evaluate_split.npz and tests/golden/fit_decisions.npz by running the REFERENCE's own
``evaluate.evaluate`` / ``train.evaluate_model`` / ``train.train_model`` (dev container only; see generate_fixtures.py).

    python tests/golden/generate_eval_fixtures.py        # needs /root/reference (read-only)

evaluate_split.npz: fixed logits for 23 pages in three loader batches of at most 10 (case "a") and a small second case
("b") in which a listed domain has no evaluated page; the reference's img_acc / class_acc for k = 1 and 3, its macro
accuracy, the texts of both CSV files and of its logs.

fit_decisions.npz: train.train_model with a tiny CPU model.  Two module attributes are patched around the call --
``train.evaluate_model`` (a stub returning a scripted accuracy sequence) and ``torch.save`` (a recorder that also saves);
the reference file itself is not edited.  Recorded per sequence: the epochs evaluated, the epochs saved, the number of
scheduler steps, the learning rate of every epoch under StepLR(2, 0.5) and the returned best.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_standin"))
sys.path.insert(0, REF)

import torchvision  # noqa: E402,F401  (the stand-in)
import train as ref_train  # noqa: E402
import evaluate as ref_evaluate  # noqa: E402

assert ref_train.__file__.startswith(REF), ref_train.__file__
assert ref_evaluate.__file__.startswith(REF), ref_evaluate.__file__

CLASS_NAMES = ["BG", "Price", "Title", "Image"]


def make_split(rs, counts, bias):
    """Per page: labels with one box of each class at random positions, standard-normal logits with ``bias`` added to
    the labelled box in its own column."""
    labels, logits = [], []
    for n in counts:
        lab = np.zeros(n, dtype=np.int64)
        lab[rs.permutation(n)[:3]] = [1, 2, 3]
        lg = rs.standard_normal((n, 4)).astype(np.float32)
        for c in (1, 2, 3):
            lg[np.nonzero(lab == c)[0][0], c] += np.float32(bias)
        labels.append(lab)
        logits.append(lg)
    return labels, logits


def run_reference(tag, counts, names, webpage_info, domains, bias, seed, batch=10):
    rs = np.random.RandomState(seed)
    labels, logits = make_split(rs, counts, bias)
    P = len(counts)
    loader, per_batch = [], []
    for s in range(0, P, batch):
        idx = list(range(s, min(s + batch, P)))
        n = sum(counts[i] for i in idx)
        bb = np.zeros((n, 5), dtype=np.float32)
        bb[:, 0] = np.concatenate([np.full(counts[i], j, dtype=np.float32) for j, i in enumerate(idx)])
        bb[:, 1:] = rs.uniform(0, 30, (n, 4)).astype(np.float32)
        loader.append((names[idx], torch.zeros(len(idx), 3, 4, 4), torch.from_numpy(bb), torch.zeros(n, 0),
                       torch.zeros(n, 0, dtype=torch.int64), torch.from_numpy(np.concatenate([labels[i] for i in idx]))))
        per_batch.append(torch.from_numpy(np.concatenate([logits[i] for i in idx])))

    class Fixed(torch.nn.Module):
        n_classes = 4
        class_names = CLASS_NAMES

        def __init__(self):
            super().__init__()
            self.calls = 0

        def forward(self, *a):
            out = per_batch[self.calls % len(per_batch)]
            self.calls += 1
            return out

    out = {}
    with tempfile.TemporaryDirectory() as d:
        log, imgwise, domwise = d + "/log.txt", d + "/imgwise.csv", d + "/domainwise.csv"
        class_acc, macro = ref_evaluate.evaluate(Fixed(), loader, "cpu", log, imgwise, webpage_info, domains, domwise)
        out["macro_acc"] = np.asarray(macro)
        out["log_evaluate"] = np.array(open(log).read())
        out["imgwise_csv"] = np.array(open(imgwise).read())
        out["domainwise_csv"] = np.array(open(domwise).read())
        for k in (1, 3):
            log_k = d + "/log_k%d.txt" % k
            img_acc, acc = ref_train.evaluate_model(Fixed(), loader, "cpu", k, "VAL", log_k)
            out["img_acc_k%d" % k], out["class_acc_k%d" % k] = img_acc, acc
            out["log_k%d" % k] = np.array(open(log_k).read())
        assert np.array_equal(out["class_acc_k1"], class_acc)
    out.update(counts=np.asarray(counts), names=names, webpage_info=webpage_info, domains=domains,
               logits=np.concatenate(logits), labels=np.concatenate(labels),
               bboxes=np.concatenate([b[2].numpy() for b in loader]))
    print(tag, "class_acc k1", out["class_acc_k1"], "k3", out["class_acc_k3"], "macro", out["macro_acc"])
    return {"%s/%s" % (tag, k): v for k, v in out.items()}


def case_evaluate_split():
    rs = np.random.RandomState(11)
    counts = rs.randint(5, 70, 23).tolist()
    counts[3], counts[17] = 4, 131
    names = np.asarray([str(i) for i in rs.permutation(9000)[:23] + 1000])
    doms = ["shop-a.com", "shop-b.org", "books.example", "market.example", "store-e.net"]
    page_dom = [doms[i] for i in rs.randint(0, 5, 23)]
    # webpage_info also lists pages that are not in the split: N_examples counts them
    extra = [(str(20000 + i), doms[i % 5]) for i in range(7)] + [("30001", "elsewhere.example")]
    info = np.asarray(list(zip(names.tolist(), page_dom)) + extra)
    info = info[rs.permutation(len(info))]
    out = run_reference("a", counts, names, info, np.asarray(doms), bias=1.9, seed=12)
    # second case: "empty.example" is a test domain whose only listed page is not evaluated
    counts_b = [9, 4, 30, 12, 7, 18]
    names_b = np.asarray(["7", "12", "3", "44", "5", "60"])
    info_b = np.asarray([("7", "x.example"), ("12", "y.example"), ("3", "x.example"), ("44", "y.example"),
                         ("5", "y.example"), ("60", "x.example"), ("99", "empty.example")])
    out.update(run_reference("b", counts_b, names_b, info_b, np.asarray(["x.example", "empty.example", "y.example"]),
                             bias=1.9, seed=13, batch=4))
    np.savez_compressed(os.path.join(HERE, "evaluate_split.npz"), **out)


# ---------------------------------------------------------------------------------------------- train.train_model
FIT_CASES = [
    # (scripted eval accuracies, repeated from the last value on; n_epochs; eval_interval)
    ([50, 60, 60, 55, 70, 1], 30, 2),                 # ties, a late improvement, an early stop at epoch 22
    ([40, 40, 40, 41, 41], 10, 3),                    # ties; n_epochs not a multiple of the interval
    ([30, 29, 28, 27, 26, 25, 24, 31, 5], 40, 1),     # six misses, an improvement, then seven misses
    ([10, 9], 20, 1),                                 # stops as early as it can
    ([5, 6, 7, 8], 7, 3),                             # runs to the end: evaluated at 1, 3, 6, 7
    ([20, 30, 25, 35, 35, 36], 16, 3),                # the last epoch is evaluated and is the best
]


class TinyModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 4)

    def forward(self, images, bboxes, additional_feats, context_indices):
        return self.lin(bboxes[:, 1:])


def case_fit_decisions():
    out = {"n_cases": np.asarray(len(FIT_CASES))}
    for i, (seq, n_epochs, interval) in enumerate(FIT_CASES):
        torch.manual_seed(i)
        model = TinyModel()
        opt = torch.optim.Adam(model.parameters(), lr=5e-4)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        n = 12
        batch = (np.asarray(["0"]), torch.zeros(1, 3, 4, 4), torch.rand(n, 5), torch.zeros(n, 0),
                 torch.zeros(n, 0, dtype=torch.int64), torch.randint(0, 4, (n,)))
        lrs, evaluated, saved = [], [], []

        class Loader:
            def __iter__(self):
                lrs.append(opt.param_groups[0]["lr"])
                return iter([batch])

        def stub(model, loader, device, k, split, log_file):
            evaluated.append(sched.last_epoch + 1)
            return None, np.asarray([0.0, float(seq[min(len(evaluated), len(seq)) - 1])])

        real_save, real_eval = torch.save, ref_train.evaluate_model

        def recording_save(obj, f, *a, **kw):
            saved.append(sched.last_epoch + 1)
            return real_save(obj, f, *a, **kw)

        with tempfile.TemporaryDirectory() as d:
            ref_train.evaluate_model, torch.save = stub, recording_save
            try:
                best = ref_train.train_model(model, Loader(), opt, sched, torch.nn.CrossEntropyLoss(reduction="sum"),
                                             n_epochs, "cpu", None, interval, d + "/log.txt", d + "/ckpt.pth")
            finally:
                ref_train.evaluate_model, torch.save = real_eval, real_save
        tag = "c%d/" % i
        out.update({tag + "seq": np.asarray(seq, dtype=np.float64), tag + "n_epochs": np.asarray(n_epochs),
                    tag + "eval_interval": np.asarray(interval), tag + "evaluated": np.asarray(evaluated),
                    tag + "saved": np.asarray(saved), tag + "scheduler_steps": np.asarray(sched.last_epoch),
                    tag + "lr": np.asarray(lrs, dtype=np.float64), tag + "best": np.asarray(float(best))})
        print("fit case %d: evaluated %s saved %s epochs %d steps %d best %s" % (i, evaluated, saved, len(lrs),
                                                                                  sched.last_epoch, best))
    np.savez_compressed(os.path.join(HERE, "fit_decisions.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    case_evaluate_split()
    case_fit_decisions()
