"""Evaluation of a whole resident split and the epoch loop around the train step (the outer half of the reference).

``evaluate_split`` is ``train.evaluate_model`` (train.py:99-171) over a ``pipeline.DeviceDataset``: per batch the
eval-mode forward and ONE cova_eval_page_ranks launch that scatters the rank of every labelled box into split-resident
tables; after the last batch one device-to-host copy.  ``EvalReport`` (host only) turns the tables into the reference's
outputs: ``img_acc`` / ``class_acc`` for any k, the image-wise and domain-wise files and the macro accuracy of
``evaluate.evaluate`` (evaluate.py:14-84), the log lines.

``fit`` is ``train.train_model`` (train.py:9-96): epochs of ``train_step`` fed by the dataset, evaluation at epoch 1,
every ``eval_interval`` epochs and at the last one, save-best, patience, the learning-rate schedule, reload-best.  Its
decisions live in the host-only ``EpochController``.

Table values: ``>= 0`` the rank of the labelled box (0 = best), ``-1`` the page has no box of the class, ``-2`` the page
was not evaluated.

``decode="joint"`` (opt-in everywhere; the default ``"column"`` is the reference's arg-max per class column): every page
of the data holds exactly one box of each non-background class, and cova_page_joint_decode picks one DISTINCT box per
class, the most probable such labelling under the model's per-box softmax (``score="map"``).  ``evaluate_split`` then
also fills ``joint_top1`` (the chosen box), ``joint_hit`` (1 hit, 0 miss, -1 no box of the class, -2 not evaluated) and
``joint_gap`` (float64: best total minus the second best, -1.0 not evaluated); ``predict_split`` is the label-free call.
At most 7 classes (the kernel enumerates up to 7^6 assignments a page): more is a ValueError.
"""
import collections
import contextlib
import time

import numpy as np
import torch

from . import engine
from .trainer import LossMetrics, shard_pages

NOT_EVALUATED, UNLABELLED = -2, -1
CLASS_NAMES = ("BG", "Price", "Title", "Image")            # constants.py of the reference


def _names(class_names, nc):
    if class_names is None:
        class_names = CLASS_NAMES if nc == len(CLASS_NAMES) else ["class%d" % c for c in range(nc)]
    if len(class_names) != nc:
        raise ValueError("class_names must hold n_classes = %d names" % nc)
    return list(class_names)


class EvalReport:
    """Host-side result of one split: ``ranks`` / ``top1`` int32 [P, NC-1] (module docstring for the values) and the
    page names ``img_ids`` [P].  ``loss`` / ``confusion`` / ``metrics`` are set when the split ran ``with_loss``."""

    def __init__(self, ranks, top1=None, img_ids=None, metrics=None, seconds=0.0, joint_top1=None, joint_hit=None,
                 joint_gap=None):
        self.ranks = np.ascontiguousarray(ranks, dtype=np.int32)
        if self.ranks.ndim != 2 or self.ranks.shape[1] < 1:
            raise ValueError("ranks must be [P, n_classes - 1], got shape %s" % (self.ranks.shape,))
        P = self.ranks.shape[0]
        self.top1 = None if top1 is None else np.ascontiguousarray(top1, dtype=np.int32)
        if self.top1 is not None and self.top1.shape != self.ranks.shape:
            raise ValueError("top1 must have the shape of ranks")
        self.img_ids = np.asarray([str(i) for i in range(P)]) if img_ids is None else np.asarray(img_ids)
        if self.img_ids.shape != (P,):
            raise ValueError("img_ids must hold one name per page")
        self.metrics, self.seconds = metrics, float(seconds)
        # the tables of decode="joint" (module docstring), None on a report that ran without it
        self.joint_top1 = None if joint_top1 is None else np.ascontiguousarray(joint_top1, dtype=np.int32)
        self.joint_hit = None if joint_hit is None else np.ascontiguousarray(joint_hit, dtype=np.int32)
        self.joint_gap = None if joint_gap is None else np.ascontiguousarray(joint_gap, dtype=np.float64)
        for name in ("joint_top1", "joint_hit"):
            t = getattr(self, name)
            if t is not None and t.shape != self.ranks.shape:
                raise ValueError("%s must have the shape of ranks" % name)
        if self.joint_gap is not None and self.joint_gap.shape != (P,):
            raise ValueError("joint_gap must hold one value per page")
        self.loss = None if metrics is None else metrics["loss"]
        self.confusion = None if metrics is None else metrics["confusion"]

    @property
    def n_classes(self):
        return self.ranks.shape[1] + 1

    @property
    def evaluated(self):
        """bool [P]: the page was in a batch of the split (of any rank, once the tables are merged)."""
        return (self.ranks != NOT_EVALUATED).any(axis=1)

    @property
    def unlabelled(self):
        """int64 [NC] (entry 0 is 0): evaluated pages without a box of the class.  They score a miss."""
        out = np.zeros(self.n_classes, dtype=np.int64)
        out[1:] = (self.ranks[self.evaluated] == UNLABELLED).sum(axis=0)
        return out

    @staticmethod
    def merge(reports):
        """The tables of several ranks folded by maximum (what evaluate_split's all-reduce does on the device)."""
        reports = list(reports)
        ranks = np.maximum.reduce([r.ranks for r in reports])
        def fold(name):
            tabs = [getattr(r, name) for r in reports]
            return None if any(t is None for t in tabs) else np.maximum.reduce(tabs)
        return EvalReport(ranks, fold("top1"), reports[0].img_ids, seconds=max(r.seconds for r in reports),
                          joint_top1=fold("joint_top1"), joint_hit=fold("joint_hit"), joint_gap=fold("joint_gap"))

    def hits(self, k=1, decode="column"):
        """bool [P, NC-1]: the labelled box is among the k best of its column; with ``decode="joint"`` (k must be 1, and
        the report must carry the joint tables, else ValueError): the labelled box is the joint choice of its class."""
        if int(k) < 1:
            raise ValueError("k must be >= 1")
        if decode == "joint":
            if int(k) != 1:
                raise ValueError("decode=\"joint\" decides one box per class: k must be 1, got %r" % (k,))
            if self.joint_hit is None:
                raise ValueError("this report carries no joint tables: run evaluate_split(decode=\"joint\")")
            return self.joint_hit == 1
        if decode != "column":
            raise ValueError("decode must be one of %s, got %r" % (engine.DECODE_MODES, decode))
        return (self.ranks >= 0) & (self.ranks < int(k))

    def img_acc(self, k=1, decode="column"):
        """train.py:156: int32 [n_evaluated, NC] rows [img_id, hit ...], pages in dataset order."""
        ev = self.evaluated
        try:
            ids = np.array(self.img_ids[ev].tolist(), dtype=np.int32).reshape(-1)
        except (ValueError, TypeError, OverflowError):
            raise ValueError("img_acc needs integer-like page names (train.py:156 builds an int32 array), got e.g. %r"
                             % (self.img_ids[ev][:1].tolist(),))
        return np.concatenate([ids.reshape(-1, 1), self.hits(k, decode)[ev].astype(np.int32)], axis=1)

    def class_acc(self, k=1, decode="column"):
        """train.py:157-158: float64 [NC], entry 0 is 0, percentages over the evaluated pages."""
        out = np.zeros(self.n_classes)
        out[1:] = self.hits(k, decode)[self.evaluated].astype(np.int32).mean(0) * 100
        return out

    # ---- evaluate.py:53-78
    def domainwise(self, webpage_info, domains, k=1, decode="column"):
        """-> (n_examples int64 [D], acc float64 [D, NC-1]) for the domains in order.  ``webpage_info``: [*, 2] rows
        (img_id, domain).  N_examples counts the rows of ``webpage_info``; the accuracy is over the evaluated pages of
        the domain (NaN when there is none)."""
        info = np.asarray(webpage_info)
        img_acc = self.img_acc(k, decode)
        n, acc = [], []
        for domain in np.asarray(domains).reshape(-1):
            domain_imgs = info[np.isin(info[:, 1], domain), 0].astype(np.int32)
            with np.errstate(invalid="ignore", divide="ignore"):
                rows = img_acc[np.isin(img_acc[:, 0], domain_imgs), 1:]
                acc.append(rows.mean(0) * 100 if rows.shape[0] else np.full(self.n_classes - 1, np.nan))
            n.append(len(domain_imgs))
        return np.asarray(n, dtype=np.int64), np.asarray(acc, dtype=np.float64).reshape(len(n), self.n_classes - 1)

    def _domain_rows(self, webpage_info, domains, k, decode="column"):
        n, acc = self.domainwise(webpage_info, domains, k, decode)
        return [(str(d), int(m), ["%.2f" % v for v in a]) for d, m, a in zip(np.asarray(domains).reshape(-1), n, acc)]

    def macro_acc(self, webpage_info, domains, k=1, decode="column"):
        """evaluate.py:71-78: float64 [NC], entry 0 is 0: the float32 mean over the domains of the two-decimal TEXT of
        each domain's accuracy (the reference reads its own CSV back)."""
        rows = self._domain_rows(webpage_info, domains, k, decode)
        out = np.zeros(self.n_classes)
        with np.errstate(invalid="ignore"):
            out[1:] = np.asarray([r[2] for r in rows]).reshape(len(rows), -1).astype(np.float32).mean(0)
        return out

    def write_imgwise_csv(self, path, k=1, class_names=None, decode="column"):
        """evaluate.py:35-42, byte for byte."""
        names = _names(class_names, self.n_classes)
        np.savetxt(path, self.img_acc(k, decode), "%s" + ",%.2f" * (self.n_classes - 1), ",",
                   header="img_id," + ",".join("%s_acc" % n.lower() for n in names[1:]), comments="")

    def write_domainwise_csv(self, path, webpage_info, domains, k=1, class_names=None, decode="column"):
        """evaluate.py:48-69, byte for byte."""
        names = _names(class_names, self.n_classes)
        with open(path, "w") as f:
            f.write("Domain,N_examples,%s\n" % ",".join(names[1:]))
            for d, n, texts in self._domain_rows(webpage_info, domains, k, decode):
                f.write("%s,%d,%s\n" % (d, n, ",".join(texts)))

    def log_lines(self, split_name="VAL", k=1, class_names=None, decode="column"):
        """The lines of train.py:160-169 (the last one is empty)."""
        names, acc = _names(class_names, self.n_classes), self.class_acc(k, decode)
        lines = ["[%s] Avg_class_Accuracy: %.2f%% (%.2fs)" % (split_name, acc[1:].mean(), self.seconds)]
        lines += ["%s top-%d-Acc: %.2f%%" % (names[c], k, acc[c]) for c in range(1, self.n_classes)]
        return lines + [""]

    def macro_log_lines(self, webpage_info, domains, k=1, class_names=None, decode="column"):
        """The lines of evaluate.py:79-82."""
        names, macro = _names(class_names, self.n_classes), self.macro_acc(webpage_info, domains, k, decode)
        return ["%s Macro Acc: %.2f%%" % (names[c], macro[c]) for c in range(1, self.n_classes)]


def eval_plan(n_pages, batch_size, rank=0, world_size=1):
    """Page ids of every evaluation batch of this rank: the rank's ``shard_pages`` range of the split in dataset order,
    cut into batches; the short last batch is kept and a rank may have fewer batches than another, or none."""
    n_pages, batch_size, rank, world_size = int(n_pages), int(batch_size), int(rank), int(world_size)
    if n_pages < 0 or batch_size < 1 or world_size < 1 or not (0 <= rank < world_size):
        raise ValueError("eval_plan: need n_pages >= 0, batch_size >= 1 and 0 <= rank < world_size")
    lo, hi = shard_pages(n_pages, rank, world_size)
    return [np.arange(s, min(s + batch_size, hi), dtype=np.int64) for s in range(lo, hi, batch_size)]


def _read_tables(blob):
    """The one device-to-host copy of a split."""
    return blob.cpu().numpy()


@torch.no_grad()
def evaluate_split(trainer, dataset, batch_size=10, rank=0, world_size=1, group=None, with_loss=False, prefetch=True,
                   merge=True, features=None, decode="column", score="map"):
    """Evaluate every page of ``dataset`` (a DeviceDataset) in dataset order, nothing shuffled, sampled or dropped
    (datasets.py:227-258) -> EvalReport.  Under data parallelism every rank calls this with its ``rank``; the tables are
    merged by one all_reduce(MAX) (``merge=False`` leaves a rank's own tables: other ranks' pages stay -2, see
    EvalReport.merge).  ``with_loss`` also runs cova_ce_loss_fwd with the trainer's criterion options into counters of the
    report's own (``trainer.metrics`` is not touched).  No host read before the copy at the end.
    ``features`` (a features.FeatureCache of this trainer's conv stack over ``dataset``): checked once on entry (one
    host read), then every batch takes its visual rows from the table: no page gather, conv stack or RoI op.
    ``decode="joint"`` (``score``: "map" or "logit"; at most 7 classes, else ValueError): one more launch per batch,
    cova_page_joint_decode, fills ``joint_top1`` / ``joint_hit`` / ``joint_gap`` of the report (module docstring); they sit
    behind the other tables in the same buffer, are merged by the same MAX all-reduce and come back in the same copy.
    ``ranks`` and ``top1`` are what ``decode="column"`` gives."""
    start = time.time()
    dev, nc, P = trainer.device, int(trainer.cfg["n_classes"]), len(dataset)
    if nc < 2:
        raise ValueError("evaluation needs at least one non-background class")
    mode, joint = engine.check_decode(decode, score, nc), decode == "joint"
    if features is not None:
        features.check(trainer, dataset)
    plan = eval_plan(P, batch_size, rank, world_size)
    lo, hi = shard_pages(P, rank, world_size)
    m = nc * nc + 4
    # one int32 buffer = [metrics as int64 | rank table | top1 table]: one copy brings everything back
    n_tab = 2 * P * (nc - 1)
    # (joint: two more int32 tables, then the float64 gaps; every part is an even number of int32 words, so 8-byte aligned)
    blob = torch.empty(2 * m + n_tab + (n_tab + 2 * P if joint else 0), dtype=torch.int32, device=dev)
    metrics_buf, tables = blob[:2 * m].view(torch.int64), blob[2 * m:2 * m + n_tab].view(2, P, nc - 1)
    metrics_buf.zero_()
    tables.fill_(NOT_EVALUATED)
    if joint:
        jtab = blob[2 * m + n_tab:2 * m + 2 * n_tab].view(2, P, nc - 1)
        jgap = blob[2 * m + 2 * n_tab:].view(torch.float64)
        jtab.fill_(NOT_EVALUATED)
        jgap.fill_(-1.0)
    ids32 = torch.from_numpy(np.arange(lo, hi, dtype=np.int32)).to(dev)
    opts = ws = None
    if with_loss:
        opts = trainer._criterion() or engine.check_loss_options(nc)
    pos = 0
    for ids, batch in zip(plan, dataset.batches(batch_size, order=np.arange(lo, hi, dtype=np.int64), world_size=1,
                                                prefetch=prefetch, features=features)):
        B = int(ids.shape[0])
        logits, _ = trainer.predict(batch)
        engine.call("cova_eval_page_ranks", logits, batch["labels"], batch["page_start"], ids32[pos:pos + B], B, nc, P,
                    tables[0], tables[1])
        if joint:
            engine.call("cova_page_joint_decode", logits, batch["labels"], batch["page_start"], ids32[pos:pos + B], B, nc,
                        P, mode, jtab[0], jtab[1], jgap)
        if with_loss:
            n_ws = engine.query("cova_ce_loss_workspace_doubles", logits.shape[0])
            if ws is None or ws.numel() < n_ws:
                ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
            engine.ce_loss_fwd(logits, batch["labels"], trainer.class_weight, opts, metrics_buf, want_pred=False,
                               workspace=ws)
        pos += B
    if world_size > 1 and merge:
        import torch.distributed as dist
        dist.all_reduce(tables, op=dist.ReduceOp.MAX, group=group)
        if joint:                            # unwritten rows hold -2 / -1.0, below everything a page can get
            dist.all_reduce(jtab, op=dist.ReduceOp.MAX, group=group)
            dist.all_reduce(jgap, op=dist.ReduceOp.MAX, group=group)
        if with_loss:                        # the counts and the two float64 sums add up over the ranks, in place
            dist.all_reduce(metrics_buf[:nc * nc + 2], op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(metrics_buf[nc * nc + 2:].view(torch.float64), op=dist.ReduceOp.SUM, group=group)
    host = _read_tables(blob)
    tab = host[2 * m:2 * m + n_tab].reshape(2, P, nc - 1)
    jkw = {}
    if joint:
        jt = host[2 * m + n_tab:2 * m + 2 * n_tab].reshape(2, P, nc - 1)
        jkw = dict(joint_top1=jt[0], joint_hit=jt[1], joint_gap=host[2 * m + 2 * n_tab:].view(np.float64))
    metrics = None
    if with_loss:
        mh = host[:2 * m].view(np.int64)
        metrics = LossMetrics.decode(mh[:nc * nc + 2], mh[nc * nc + 2:].view(np.float64), nc,
                                     trainer.loss_options["loss_reduction"] == "mean")
    return EvalReport(tab[0], tab[1], dataset.img_ids, metrics=metrics, seconds=time.time() - start, **jkw)


@torch.no_grad()
def predict_split(trainer, dataset, batch_size=10, decode="joint", score="map", features=None, rank=0, world_size=1,
                  group=None):
    """Which boxes are the price, the title and the image of every page: the decision of ``evaluate_split`` without
    labels -> (boxes int32 [P, NC-1] page-local indices, -1 on an empty page; gap float64 [P] or None).
    ``decode="joint"``: per batch the eval-mode forward and one cova_page_joint_decode launch with labels = NULL and
    hit = NULL; ``gap`` is the distance from the best to the second-best assignment (+inf when there is no other), the
    confidence to abstain on.  ``decode="column"``: the ``top1`` of cova_eval_page_ranks (the arg-max of every column,
    which may name one box for two classes) and ``gap`` None.  Pages of other ranks are merged by one all-reduce(MAX);
    one device-to-host copy at the end, no host read before it (``features``: as evaluate_split)."""
    dev, nc, P = trainer.device, int(trainer.cfg["n_classes"]), len(dataset)
    if nc < 2:
        raise ValueError("prediction needs at least one non-background class")
    mode, joint = engine.check_decode(decode, score, nc), decode == "joint"
    if features is not None:
        features.check(trainer, dataset)
    plan = eval_plan(P, batch_size, rank, world_size)
    lo, hi = shard_pages(P, rank, world_size)
    n_tab = P * (nc - 1) + (P * (nc - 1)) % 2                  # an even number of int32 words in front of the gaps
    blob = torch.empty(n_tab + 2 * P if joint else 2 * n_tab, dtype=torch.int32, device=dev)
    boxes = blob[:P * (nc - 1)].view(P, nc - 1)
    blob.fill_(NOT_EVALUATED)
    if joint:
        gaps = blob[n_tab:].view(torch.float64)
        gaps.fill_(-1.0)
    else:
        ranks = blob[n_tab:n_tab + P * (nc - 1)].view(P, nc - 1)
    ids32 = torch.from_numpy(np.arange(lo, hi, dtype=np.int32)).to(dev)
    pos = 0
    for ids, batch in zip(plan, dataset.batches(batch_size, order=np.arange(lo, hi, dtype=np.int64), world_size=1,
                                                features=features)):
        B = int(ids.shape[0])
        logits, _ = trainer.predict(batch)
        if joint:
            engine.call("cova_page_joint_decode", logits, None, batch["page_start"], ids32[pos:pos + B], B, nc, P, mode,
                        boxes, None, gaps)
        else:
            engine.call("cova_eval_page_ranks", logits, batch["labels"], batch["page_start"], ids32[pos:pos + B], B, nc,
                        P, ranks, boxes)
        pos += B
    if world_size > 1:
        import torch.distributed as dist
        dist.all_reduce(boxes, op=dist.ReduceOp.MAX, group=group)
        if joint:
            dist.all_reduce(gaps, op=dist.ReduceOp.MAX, group=group)
    host = _read_tables(blob)
    out = host[:P * (nc - 1)].reshape(P, nc - 1)
    return out, (host[n_tab:].view(np.float64) if joint else None)


# ------------------------------------------------------------------------------------------------ the epoch loop
class EpochController:
    """The decisions of train.py:29-31,72-89 on the host: when to evaluate, what counts as the best, when to stop.

    One difference from the reference: ``patience_count`` starts at 0.  The reference leaves it unset until the first
    improvement and raises (UnboundLocalError) if the very first evaluation is 0.0; here that is "no improvement"."""

    def __init__(self, n_epochs, eval_interval=3, patience=7):
        self.n_epochs, self.eval_interval, self.patience = int(n_epochs), int(eval_interval), int(patience)
        if self.n_epochs < 0 or self.eval_interval < 1 or self.patience < 1:
            raise ValueError("EpochController: need n_epochs >= 0, eval_interval >= 1 and patience >= 1")
        self.best_eval_acc, self.best_epoch, self.patience_count, self.stopped = 0.0, None, 0, False

    def should_evaluate(self, epoch):
        return epoch == 1 or epoch % self.eval_interval == 0 or epoch == self.n_epochs

    def update(self, epoch, eval_acc):
        """-> (is_best, stop) for the evaluation result of ``epoch``."""
        if eval_acc > self.best_eval_acc:                 # strictly: a tie is no improvement
            self.best_eval_acc, self.best_epoch, self.patience_count = float(eval_acc), int(epoch), 0
            return True, False
        self.patience_count += 1
        self.stopped = self.patience_count >= self.patience
        return False, self.stopped


def step_lr(step_size, gamma=0.1):
    """torch.optim.lr_scheduler.StepLR(step_size, gamma) (main.py:136) as a factor on the initial lr: after ``epoch``
    completed epochs the factor is gamma ** (epoch // step_size)."""
    step_size, gamma = int(step_size), float(gamma)
    if step_size < 1:
        raise ValueError("step_size must be >= 1")
    return lambda epoch: gamma ** (int(epoch) // step_size)


FitResult = collections.namedtuple("FitResult", "best_eval_acc best_epoch epochs_run stopped_early history")


def _log(log_file, lines):
    if log_file is not None:
        with open(log_file, "a") as f:
            f.write("".join(line + "\n" for line in lines))


def fit(trainer, train_set, val_set, n_epochs, batch_size, sampling_fraction=0.9, seed=0, eval_interval=3, patience=7,
        lr_schedule=None, checkpoint=None, log_file=None, k=1, rank=0, world_size=1, group=None, class_names=None,
        train_features=None, val_features=None, augment=None, use_average=False, decode="column", decode_score="map"):
    """train.train_model: ``n_epochs`` epochs of ``trainer.train_step`` over ``train_set`` (shuffled, background boxes
    sampled), ``evaluate_split`` on ``val_set`` at epoch 1, every ``eval_interval`` epochs and at the last epoch,
    save-best / patience / reload-best -> FitResult.

    The epoch's loss (per scored box), accuracy and box count come from ``trainer.metrics`` (read and reset once per
    epoch; the counters are also reset on entry), so the trainer must have been built with ``track_metrics=True``.
    ``lr_schedule``: epoch -> factor on every group's lr as it was on entry, applied after each completed epoch and not
    after the one that stops early (scheduler.step(), train.py:91).  Rank 0 appends the reference's lines to
    ``log_file`` and keeps the best state_dict (``torch.save`` to ``checkpoint``, else a clone in memory); the best is
    reloaded at the end on every rank.  Every rank sees the same merged tables and takes the same decisions.
    ``train_features`` / ``val_features`` (features.FeatureCache over ``train_set`` / ``val_set``, for a trainer whose
    conv stack is frozen with its BatchNorms in eval mode): checked once on entry; the steps and the evaluations then
    take the visual rows from the tables.
    ``augment`` (a pipeline.PageAugment): the TRAINING batches of every epoch are augmented (keyed by ``epoch``, so no two
    epochs show a page alike); ``evaluate_split`` never is.  Not with ``train_features`` (ValueError).
    ``use_average`` (a trainer built with ``average=``, else ValueError): every validation runs inside
    ``trainer.averaged_weights()`` and the best state kept or saved is ``averaged_state_dict()``, so save-best and
    patience follow the averaged model; an evaluation before the average has started (``n_averaged == 0``) uses the
    live weights and state.  The history's ``averaged`` says which it was.  The final reload goes through
    ``load_state_dict``, after which live parameters and average both hold the best state.
    A trainer built with ``accumulate_steps`` n > 1: ``trainer.flush()`` follows the last batch of every epoch, before the
    metrics are read, before any evaluation and before ``lr_schedule`` applies, so an epoch whose batch count is no
    multiple of n ends with a smaller update and no gradient crosses an epoch or an evaluation.  The history's ``updates``
    is the number of parameter updates of the epoch.
    ``decode="joint"`` (``decode_score``: "map" or "logit"; k must be 1, at most 7 classes, else ValueError): every
    validation runs ``evaluate_split(decode="joint")`` and ``class_acc`` / ``eval_acc``, the logged lines, save-best and
    patience follow the joint hits.  The history's ``decode`` records the mode."""
    # (the class count limits the joint mode alone; the default asks nothing of the trainer here, as before)
    engine.check_decode(decode, decode_score, int(trainer.cfg["n_classes"]) if decode == "joint" else 2, k)
    dec_kw = {} if decode == "column" else dict(decode=decode, score=decode_score)
    rep_kw = {} if decode == "column" else dict(decode=decode)
    if use_average and trainer.average is None:
        raise ValueError("use_average needs a trainer built with average=\"ema\" or \"swa\"")
    if augment is not None and train_features is not None:
        raise ValueError("augment cannot be combined with train_features: the cached rows were pooled from unaugmented "
                         "pixels")
    if trainer.metrics is None:
        raise ValueError("fit needs a trainer built with track_metrics=True (the epoch's loss and accuracy are read "
                         "from trainer.metrics)")
    if train_features is not None:
        train_features.check(trainer, train_set)
    if val_features is not None:
        val_features.check(trainer, val_set)
    ctl = EpochController(n_epochs, eval_interval, patience)
    nc = int(trainer.cfg["n_classes"])
    names = _names(class_names, nc)
    base_lr = [g["lr"] for g in trainer.param_groups]
    best_state, history, epochs_run = None, [], 0
    aug_kw = {} if augment is None else dict(augment=augment)
    trainer.metrics.reset()
    accumulating = getattr(trainer, "accumulate_steps", 1) > 1
    for epoch in range(1, ctl.n_epochs + 1):
        first_update = trainer.update_count if accumulating else 0
        start, updates = time.time(), 0
        for batch in train_set.batches(batch_size, shuffle=True, sampling_fraction=sampling_fraction, seed=seed,
                                       epoch=epoch, rank=rank, world_size=world_size, features=train_features, **aug_kw):
            trainer.train_step(batch)
            updates += 1                                  # (one update per batch unless the trainer accumulates)
        if accumulating:
            trainer.flush()
            updates = trainer.update_count - first_update
        m = trainer.metrics.read()
        trainer.metrics.reset()
        n, den = m["kept"], m["loss_denominator"]
        rec = dict(epoch=epoch, loss=m["loss_numerator"] / den if den > 0 else 0.0,
                   accuracy=100.0 * float(np.trace(m["confusion"])) / n if n else 0.0, boxes=n,
                   lr=[g["lr"] for g in trainer.param_groups], eval_acc=None, class_acc=None, is_best=False,
                   averaged=False, updates=updates, decode=decode)
        rec["seconds"] = time.time() - start
        if rank == 0:
            _log(log_file, ["Epoch: %2d  Loss: %.4f  Accuracy: %.2f%%  (%.2fs)"
                            % (epoch, rec["loss"], rec["accuracy"], rec["seconds"])])
        history.append(rec)
        epochs_run = epoch
        if ctl.should_evaluate(epoch):
            rec["averaged"] = bool(use_average) and trainer.average.n_averaged > 0
            with trainer.averaged_weights() if rec["averaged"] else contextlib.nullcontext():
                report = evaluate_split(trainer, val_set, rank=rank, world_size=world_size, group=group,
                                        features=val_features, **dec_kw)
            rec["class_acc"] = report.class_acc(k, **rep_kw)
            rec["eval_acc"] = float(rec["class_acc"][1:].mean())
            if rank == 0:
                _log(log_file, report.log_lines("VAL", k, names, **rep_kw))
            rec["is_best"], stop = ctl.update(epoch, rec["eval_acc"])
            if rec["is_best"] and rank == 0:
                best_state = trainer.averaged_state_dict() if rec["averaged"] else trainer.state_dict()
                if checkpoint is not None:
                    torch.save(best_state, checkpoint)
                    best_state = None
            if stop:
                break
        if lr_schedule is not None:
            factor = float(lr_schedule(epoch))
            for g, lr in zip(trainer.param_groups, base_lr):
                g["lr"] = lr * factor
    if ctl.best_epoch is not None:
        if rank != 0:
            best_state = trainer.state_dict()             # the keys every rank validates; rank 0's values arrive
        elif checkpoint is not None:
            best_state = torch.load(checkpoint, map_location=trainer.device)
        trainer.load_state_dict(best_state, broadcast=world_size > 1)
    return FitResult(ctl.best_eval_acc, ctl.best_epoch, epochs_run, ctl.stopped, history)
