"""Training step of the hot path (train.py:42-60) as one object: forward, CE-sum, backward,
data-parallel gradient exchange, Adam -- all device work through libcova_hip.so, the gradient
exchange through torch.distributed (backend "nccl" == RCCL over xGMI on ROCm).

Data parallelism: pages are independent units, so each rank takes whole
pages; the model (1.6 M parameters) is replicated.  Every parameter lives in ONE flat fp32 buffer
and every gradient in ONE flat bucket, so a step needs exactly one all-reduce (6.47 MB, latency
bound on xGMI) and one Adam launch.  The loss is a SUM over boxes (main.py:139), so SUM-reduced
gradients equal the single-device large-batch gradient except for BatchNorm, whose batch
statistics stay per-rank (standard DDP behaviour; the reference has no SyncBN).  ``sync_bn=True``
switches on the exact large-batch mode: every BatchNorm statistic row is summed over the ranks
(engine.StatSync, 2*C floats per message), after which a data-parallel step equals the
single-device step on the concatenated batch.
"""
from collections import OrderedDict, namedtuple

import contextlib
import numbers
import os

import torch

from . import engine
from .weights import (PAGE_ATTENTION_GEO_KEY, PAGE_ATTENTION_KEY, PAGE_ENCODER_INPUT_KEY, PAGE_READOUT_KEYS, SPEC_OPTIONS,
                      check_attention_dropout, page_encoder_layer_prefix, page_options, state_dict_spec)

_BUF_SUFFIX = ("running_mean", "running_var", "num_batches_tracked")


def _page_encoder_extras(cfg, state_dict, said):
    """The page encoder's own part of HotPathTrainer._check_page_layers: its depth and its feed-forward width."""
    L, M = cfg["page_encoder_layers"], cfg["page_encoder_ffn_dim"]
    depth = 0
    while page_encoder_layer_prefix(depth) + "qkv.weight" in state_dict:
        depth += 1
    if depth != L:
        raise ValueError("%s page_encoder_layers=%d, the state_dict holds %d layer(s) under page_encoder.layers "
                         "(page_encoder_layers=%d): a checkpoint loads into the page encoder it was trained with only"
                         % (said, L, depth, depth))
    for l in range(L):
        k = page_encoder_layer_prefix(l) + "ffn1.weight"
        w = state_dict.get(k)
        if torch.is_tensor(w) and (w.dim() != 2 or w.shape[0] != M):
            raise ValueError("%s page_encoder_ffn_dim=%d, the state_dict's %s has shape %s (page_encoder_ffn_dim=%s)"
                             % (said, M, k, tuple(w.shape), w.shape[0] if w.dim() == 2 else "?"))


# HotPathTrainer._check_page_layers, per page layer: (width option, the layer in words, key prefix, the keys a checkpoint
# with the layer holds (the first one is probed: ITS rows / ``rows`` are the option's value), rows, geometry = (option,
# heads option, cfg -> the geometry weights' keys) or None, the layer's own further checks or None)
_PAGE_CHECKS = (
    ("page_context_dim", "a page readout", "page_readout.", PAGE_READOUT_KEYS, 1, None, None),
    ("page_attention_dim", "page attention", "page_attention.", (PAGE_ATTENTION_KEY,), 3,
     ("page_attention_geometry", "page_attention_heads", lambda cfg: (PAGE_ATTENTION_GEO_KEY,)), None),
    ("page_encoder_dim", "a page encoder", "page_encoder.", (PAGE_ENCODER_INPUT_KEY,), 1,
     ("page_encoder_geometry", "page_encoder_heads",
      lambda cfg: [page_encoder_layer_prefix(l) + "geometry.weight" for l in range(cfg["page_encoder_layers"])]),
     _page_encoder_extras),
)


def is_param_key(k):
    return not k.endswith(_BUF_SUFFIX)


class FlatBucket:
    """One contiguous fp32 buffer with a named view per tensor (device agnostic)."""

    def __init__(self, shapes, device):
        self.offsets, n = OrderedDict(), 0
        for k, shape in shapes.items():
            numel = int(torch.Size(shape).numel())
            self.offsets[k] = (n, numel, tuple(shape))
            n += (numel + 3) // 4 * 4           # keep every view 16-byte aligned
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        self.views = OrderedDict((k, self.flat[o:o + m].view(shape))
                                 for k, (o, m, shape) in self.offsets.items())

    def like(self):
        """A zeroed bucket of the same layout on the same device."""
        return FlatBucket(OrderedDict((k, shape) for k, (_, _, shape) in self.offsets.items()), self.flat.device)

    def all_reduce_sum(self, group=None):
        """One collective for the whole bucket."""
        import torch.distributed as dist
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)

    def split_at(self, first_key):
        """Flat offset at which tensor ``first_key`` starts (the bucket keeps state_dict order)."""
        return self.offsets[first_key][0]

    def all_reduce_range(self, lo, hi, group=None, async_op=False):
        """SUM all-reduce of flat[lo:hi]; with async_op the collective runs on the backend's own
        stream (RCCL) and the returned work handle must be waited on before the range is read."""
        import torch.distributed as dist
        return dist.all_reduce(self.flat[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=async_op)


def _named_by(name, entries):
    """state_dict key / BatchNorm prefix ``name`` is named by one of ``entries`` (keys or key prefixes)."""
    return any(name.startswith(e) or e.startswith(name) for e in entries)


OPTIMIZERS = ("adam", "adamw", "sgd")           # index = the algorithm code of cova_optim_step
_GROUP_HP = ("lr", "weight_decay", "betas", "eps", "momentum", "dampening", "nesterov")
_ADAM_HP = ("lr", "weight_decay", "betas", "eps")                      # the "hp" of an optimizer_state_dict


def _entries(spec):
    return (spec,) if isinstance(spec, str) else tuple(spec)


def _check_sgd_group(algorithm, hp):
    if algorithm == "sgd" and hp["nesterov"] and (hp["momentum"] <= 0 or hp["dampening"] != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")


def group_runs(offsets, n, frozen, owner):
    """Merged runs [lo, hi, group] of the flat buffer: adjacent trainable tensors of one group form one run (a run spans
    the alignment padding behind each of its views); frozen keys (``owner`` has none) split runs and are left out."""
    keys = list(offsets)
    ends = [offsets[k][0] for k in keys[1:]] + [n]
    runs = []
    for k, hi in zip(keys, ends):
        if k in frozen:
            continue
        lo, gid = offsets[k][0], owner[k]
        if runs and runs[-1][1] == lo and runs[-1][2] == gid:
            runs[-1][1] = hi
        else:
            runs.append([lo, hi, gid])
    return [tuple(r) for r in runs]


class SegmentTable:
    """The segment table of the flat-bucket kernels (csrc/optim.hip) from runs [(lo, hi, group)]: ``rows`` {lo, hi, group,
    start} with ``start`` the running length, ``total`` their summed length and ``tensor``, the int64 [-1, 4] device
    tensor the launches read: None until args() is first called, so a table nothing launches over holds no device memory."""

    def __init__(self, runs, device):
        self.rows, self.total, self.tensor, self._device = [], 0, None, device
        for lo, hi, gid in runs:
            self.rows.append((lo, hi, gid, self.total))
            self.total += hi - lo

    def args(self):
        """(seg, n_seg, total) in the order every entry point over the table takes them."""
        if self.tensor is None:
            self.tensor = torch.tensor(self.rows, dtype=torch.int64).view(-1, 4).to(self._device)
        return self.tensor, len(self.rows), self.total


def group_rows(groups, buf_exists):
    """Per parameter group the nine doubles lr, weight_decay, beta1, beta2, eps, momentum, dampening, nesterov, momentum
    buffer exists.  The column order is the ABI of cova_optim_step's ``groups`` argument (include/cova_hip.h; csrc/optim.hip
    reads h[0] .. h[8] of each row) and the message of HotPathTrainer._broadcast_groups: change it there too or not at all."""
    return [[g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"], g["momentum"], g["dampening"],
             float(g["nesterov"]), float(b)] for g, b in zip(groups, buf_exists)]


AVERAGES = ("ema", "swa")
# trainer.average: the averaging options as given and the number of parameter samples in the average so far
AverageInfo = namedtuple("AverageInfo", "kind decay warmup start every buffers n_averaged")


def average_weight(kind, decay, warmup, n_averaged):
    """``one_minus_decay`` (a double) of the cova_weight_average launch that adds a sample to an average of ``n_averaged``:
    "swa" 1 / (n_averaged + 1), the equal-weight running mean of torch's AveragedModel; "ema" 1 - d with d = ``decay``,
    or with ``warmup`` min(decay, (1 + n_averaged) / (warmup + n_averaged)): early samples weigh more while the average
    is young."""
    n = int(n_averaged)
    if kind == "swa":
        return 1.0 / (n + 1)
    d = float(decay)
    if warmup is not None:
        d = min(d, (1.0 + n) / (float(warmup) + n))
    return 1.0 - d


def check_average_options(average, decay, warmup, start, every, buffers):
    """The checked averaging options of HotPathTrainer -> AverageInfo with n_averaged 0, or None when averaging is off."""
    if average is None:
        changed = [n for n, v, d in (("average_decay", decay, 0.999), ("average_warmup", warmup, None),
                                     ("average_start", start, 0), ("average_every", every, 1),
                                     ("average_buffers", buffers, True)) if v != d]
        if changed:
            raise ValueError("%s given without average= (\"ema\" or \"swa\")" % ", ".join(changed))
        return None
    if average not in AVERAGES:
        raise ValueError("average must be None or one of %s, got %r" % (AVERAGES, average))
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError("average_decay must be in [0, 1), got %r" % (decay,))
    if warmup is not None and (int(warmup) != warmup or warmup < 1):
        raise ValueError("average_warmup must be None or an integer >= 1, got %r" % (warmup,))
    if int(start) != start or start < 0:
        raise ValueError("average_start must be an integer >= 0, got %r" % (start,))
    if int(every) != every or every < 1:
        raise ValueError("average_every must be an integer >= 1, got %r" % (every,))
    return AverageInfo(average, float(decay), None if warmup is None else int(warmup), int(start), int(every),
                       bool(buffers), 0)


ACC_OPEN, ACC_ADD, ACC_CLOSE, ACC_ADD_CLOSE = range(4)          # the modes of cova_grad_accumulate


def check_accumulate_steps(n):
    """The checked ``accumulate_steps`` of HotPathTrainer: an integer >= 1 (not a bool, a float or a string)."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError("accumulate_steps must be an integer >= 1, got %r" % (n,))
    return int(n)


def accumulate_scale(loss_reduction, m):
    """``scale`` (a double) of the launch that closes an update made from ``m`` micro-batches: 1 for the "sum"
    criterion, 1 / m for "mean" (the mean of the micro-batch means, the usual ``loss / accum_steps``)."""
    return 1.0 if loss_reduction == "sum" else 1.0 / int(m)


def shard_pages(n_pages, rank, world_size):
    """Contiguous page range [lo, hi) of this rank (whole pages only)."""
    base, rem = divmod(n_pages, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_batch(batch, rank, world_size):
    """Cut a collated batch (datasets.py:183-190 layout) into this rank's pages: boxes keep their
    order, page indices and context indices are re-based to the shard."""
    n_pages = batch["images"].shape[0]
    lo, hi = shard_pages(n_pages, rank, world_size)
    page = batch["bboxes"][:, 0]
    sel = (page >= lo) & (page < hi)
    first = int(torch.nonzero(sel)[0]) if bool(sel.any()) else 0
    bb = batch["bboxes"][sel].clone()
    bb[:, 0] -= lo
    ctx = batch["context_indices"][sel].clone()
    ctx[ctx >= 0] -= first
    return dict(images=batch["images"][lo:hi].contiguous(), bboxes=bb,
                additional_feats=batch["additional_feats"][sel].contiguous(),
                context_indices=ctx, labels=batch["labels"][sel].contiguous())


class LossMetrics:
    """Per-class counters of the criterion, accumulated on the device by cova_ce_loss_fwd (no host read per step) and
    read once per epoch: ``buf`` int64 [NC*NC + 4] = confusion[label][pred] of the kept boxes, kept boxes, bad labels, and
    the float64 running sums of the loss numerator and denominator (include/cova_hip.h)."""

    def __init__(self, n_classes, device, trainer=None):
        self.n_classes, self.trainer = int(n_classes), trainer
        self.buf = torch.zeros(self.n_classes ** 2 + 4, dtype=torch.int64, device=device)

    def reset(self):
        self.buf.zero_()

    def read(self, reduce=True):
        """-> dict of host values: confusion (numpy int64 [NC, NC], row = label, column = prediction), kept, bad_labels,
        loss (numerator / denominator, or the numerator with loss_reduction "sum"), loss_numerator, loss_denominator,
        per-class recall and precision (NaN where undefined).  One device-to-host copy; under data parallelism with
        ``reduce`` one all-reduce before it (counts travel as float64: exact below 2**53)."""
        import numpy as np
        nc, m = self.n_classes, self.n_classes ** 2
        tr = self.trainer
        if reduce and tr is not None and tr.world_size > 1:
            import torch.distributed as dist
            t = torch.cat([self.buf[:m + 2].to(torch.float64), self.buf[m + 2:].view(torch.float64)])
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=tr.group)
            host = t.cpu().numpy()
            ints, sums = np.rint(host[:m + 2]).astype(np.int64), host[m + 2:]
        else:
            host = self.buf.cpu().numpy()
            ints, sums = host[:m + 2], host[m + 2:].view(np.float64)
        return self.decode(ints, sums, nc, tr is not None and tr.loss_options["loss_reduction"] == "mean")

    @staticmethod
    def decode(ints, sums, nc, mean):
        """read()'s dict from host copies of the NC*NC + 2 integer counters and the two float64 sums."""
        import numpy as np
        m = nc * nc
        conf = np.asarray(ints[:m]).reshape(nc, nc).copy()
        num, den = float(sums[0]), float(sums[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            diag = np.diag(conf).astype(np.float64)
            recall, precision = diag / conf.sum(axis=1), diag / conf.sum(axis=0)
        return dict(confusion=conf, kept=int(ints[m]), bad_labels=int(ints[m + 1]),
                    loss=(num / den if den > 0 else 0.0) if mean else num, loss_numerator=num, loss_denominator=den,
                    recall=recall, precision=precision)


class HotPathTrainer:
    """Owns flat parameters / gradients / Adam moments on one GPU and runs training steps.

    Fine-tuning: ``frozen`` (state_dict keys or key prefixes, e.g. ("convnet.",)) get no gradient work (engine.grad_plan
    leaves out every backward stage that only they need) and are not touched by Adam (no update, no weight decay, moments
    unchanged: torch.optim.Adam's treatment of a parameter whose grad is None).  ``bn_eval`` (keys or prefixes of
    BatchNorm layers) normalise with their running statistics, leave their buffers alone and take no part in the SyncBN
    exchange.  Flat buffers, state_dict() and optimizer_state_dict() keep their layout either way.

    Optimizer ("Optimizer options"): ``optimizer`` "adam" (torch.optim.Adam, L2 added to the gradient),
    "adamw" or "sgd" (with ``momentum``, ``dampening``, ``nesterov``); ``param_groups`` [{"params": key or key prefixes,
    overrides of lr / weight_decay / betas / eps / momentum / dampening / nesterov}, ...] (unclaimed trainable keys go to a
    default group of the constructor's values, appended last); ``max_grad_norm`` clips as
    torch.nn.utils.clip_grad_norm_(params, max_grad_norm) over the trainable parameters.  These run as one cova_optim_step
    launch (plus cova_grad_norm's two launches when clipping) with no host synchronisation.  With none of them set, the
    step is today's cova_adam_step.

    Criterion ("Criterion options"): ``class_weight`` (n_classes values), ``label_smoothing``,
    ``focal_gamma`` (0 or >= 1), ``ignore_index`` (a label outside [0, n_classes): such boxes stay graph context but are
    not scored), ``loss_reduction`` "sum" | "mean" (under data parallelism the mean over the GLOBAL batch) and
    ``track_metrics`` (``trainer.metrics``: confusion counts and loss sums kept on the device).  Any of them takes the step
    from cova_ce_sum to cova_ce_loss_fwd / cova_ce_loss_bwd; with none of them set the step is today's cova_ce_sum.

    Hard-negative mining ("Hard-negative mining"): ``hard_negative_ratio`` (None: off) and
    ``hard_negative_min``: after the forward each page keeps its labelled boxes and the max(hard_negative_min,
    floor(hard_negative_ratio * labelled boxes)) background boxes with the highest plain cross-entropy; the other
    background boxes are not scored in this step (they stay graph context, ``pred`` still covers them, ``metrics`` count
    the scored rows only).  One cova_hard_negative_select launch between the forward and the criterion, which then runs
    through cova_ce_loss_fwd / cova_ce_loss_bwd; ``last_mined_labels`` / ``last_mining_counts`` hold the step's selection
    on the device.  loss() and evaluation score every row.

    Page ranking loss ("Page ranking loss"): ``page_rank_weight`` (0: off) adds ``page_rank_weight * R``
    to the step's loss, R the listwise loss of the labelled boxes among the boxes of their page, per page and class
    column: the quantity the page top-k evaluation ranks.  The criterion then runs through cova_ce_loss_fwd /
    cova_ce_loss_bwd followed by cova_page_rank_loss_fwd / cova_page_rank_loss_bwd, which add the term and its gradient
    to the pair's outputs; ``last_rank_lists`` / ``last_rank_acc`` hold the step's tables on the device.  loss()
    includes the term; ``metrics`` and evaluate_split(with_loss=) count the cross-entropy alone.

    Weight averaging ("Weight averaging"): ``average`` "ema" | "swa" (None: off) keeps an averaged copy
    of the parameters in a second flat bucket, updated at the end of optimizer_step() by one cova_weight_average launch
    over the trainable runs (a second one over the BatchNorm running statistics with ``average_buffers``), from step
    ``average_start`` on, every ``average_every`` steps, with the weight average_weight() gives (``average_decay``,
    ``average_warmup``).  ``trainer.average`` is the record, averaged_state_dict() the averaged model, and inside
    ``with trainer.averaged_weights():`` predict / evaluate / loss / evaluate_split run on it without a copy.  The
    schedule is host integers: no host read, and with ``average=None`` no tensor and no launch is added.

    Gradient accumulation ("Gradient accumulation"): ``accumulate_steps`` n > 1 makes one parameter
    update from n micro-batches: train_step() folds the gradient bucket into a second flat bucket with one
    cova_grad_accumulate launch over the trainable runs, and on the n-th micro-step closes the cycle into the gradient
    bucket and runs optimizer_step()'s path (all-reduce, clipping, update, averaging) on the accumulated gradient;
    flush() makes the update from the micro-batches pending (``accumulated``).  ``loss_reduction="sum"`` accumulates the
    plain sum (exact: the gradient of the summed loss), "mean" scales by 1 / m, the mean of the m micro-batch means, which
    is not the mean over the union when micro-batches score different numbers of boxes.  ``step_count`` counts
    micro-batches (the dropout streams), ``update_count`` parameter updates (Adam's bias correction, the averaging
    schedule).  With the default 1 no tensor and no launch is added and update_count is step_count.

    Page dropout ("Page dropout"): ``cfg["page_attention_dropout"]`` / ``cfg["page_encoder_dropout"]``
    (weights.check_page_dropout; normalised into ``self.cfg`` with the other page options, so a checkpoint's cfg carries
    them) drop inside the page attention and the page encoder in forward_backward(), on the streams
    engine.page_dropout_seed(base, layer, site) of the step's decoder base: the same seeds as CoVA.seed_dropout(), with
    or without cached features.  predict / evaluate / loss / evaluate_split and averaged_weights() run the eval-mode
    forward: the plain launches.  With both 0 no launch changes."""

    def __init__(self, cfg, state_dict, device, lr=5e-4, weight_decay=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, world_size=1, process_group=None, dropout_seed=123, sync_bn=False, frozen=(), bn_eval=(),
                 optimizer="adam", momentum=0.0, dampening=0.0, nesterov=False, param_groups=None,
                 max_grad_norm=None, norm_type=2.0, class_weight=None, label_smoothing=0.0, focal_gamma=0.0,
                 ignore_index=None, loss_reduction="sum", track_metrics=False, hard_negative_ratio=None,
                 hard_negative_min=0, page_rank_weight=0.0, average=None, average_decay=0.999, average_warmup=None,
                 average_start=0, average_every=1, average_buffers=True, accumulate_steps=1):
        self.accumulate_steps = check_accumulate_steps(accumulate_steps)
        self._avg = check_average_options(average, average_decay, average_warmup, average_start, average_every,
                                          average_buffers)
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of %s, got %r" % (OPTIMIZERS, optimizer))
        if float(norm_type) != 2.0:
            raise ValueError("norm_type must be 2.0 (the only gradient norm implemented), got %r" % (norm_type,))
        self.cfg = dict(cfg)
        if "attention_dropout" in cfg:          # (no weights: not an argument of state_dict_spec)
            self.cfg["attention_dropout"] = check_attention_dropout(cfg["attention_dropout"])
        self.cfg.update(page_options(cfg))
        self._check_page_layers(state_dict)         # (before any device work)
        self.device = torch.device(device)
        spec = state_dict_spec(**{k: self.cfg[k] for k in SPEC_OPTIONS if k in self.cfg})
        pshapes = OrderedDict((k, s) for k, s in spec if is_param_key(k))
        self.pbucket = FlatBucket(pshapes, self.device)
        self.gbucket = FlatBucket(pshapes, self.device)
        self.params, self.grads = self.pbucket.views, self.gbucket.views
        self.exp_avg = torch.zeros_like(self.pbucket.flat)
        self.exp_avg_sq = torch.zeros_like(self.pbucket.flat)
        self.buffers = {}
        # with averaging the running statistics live in one flat buffer, the batch counters in another (same keys, shapes
        # and values): the average of the statistics is then one launch with a one-row table, the counters one copy
        stat_views = self._flat_buffers(spec) if self._avg is not None else {}
        self._check_attention_mode(state_dict)
        for k, _ in spec:
            v = state_dict[k]
            if is_param_key(k):
                self.params[k].copy_(v)
            elif k in stat_views:
                self.buffers[k] = stat_views[k]
                self.buffers[k].copy_(v)
            else:
                self.buffers[k] = v.clone().to(self.device)
        self.hp = dict(lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
        self.world_size, self.group = world_size, process_group
        self.step_count, self.dropout_seed = 0, int(dropout_seed)
        self.sync_bn = bool(sync_bn) and world_size > 1
        self._setup_finetune(tuple(frozen), tuple(bn_eval))
        self._setup_optimizer(optimizer, momentum, dampening, nesterov, param_groups, max_grad_norm)
        self._setup_criterion(class_weight, label_smoothing, focal_gamma, ignore_index, loss_reduction, track_metrics)
        self._setup_mining(hard_negative_ratio, hard_negative_min)
        self._setup_rank(page_rank_weight)
        self._setup_accumulate()
        self._setup_average()
        self._ar_events = []              # (start, end) HIP events around the collective waits of optimizer_step
        self.measure_allreduce = True     # record them (up to 4096 steps; exposed_allreduce_ms() drains the list)
        if world_size > 1:
            self.broadcast_state(src=0)

    def _check_attention_mode(self, state_dict):
        """A checkpoint of the other scoring mode differs in the width of every ``attention_layer.weight`` only: name the
        mode instead of failing on a tensor size."""
        mode = self.cfg.get("attention", "gat")
        for k, p in self.params.items():
            v = state_dict.get(k) if k.endswith("attention_layer.weight") else None
            if torch.is_tensor(v) and v.numel() != p.numel():
                other = "gatv2" if p.numel() == 2 * v.numel() else "gat" if 2 * p.numel() == v.numel() else None
                raise ValueError("this trainer was configured with attention=%r (%s is %s), the state_dict holds %s%s: "
                                 "a checkpoint loads into the attention mode it was trained with only"
                                 % (mode, k, tuple(p.shape), tuple(v.shape),
                                    " (attention=%r)" % other if other and other != mode else ""))

    def _check_page_layers(self, state_dict):
        """A checkpoint loads only into the page layers it was trained with: found from its keys and shapes, and the
        message names the option instead of failing on a key or a tensor size (_PAGE_CHECKS: one row per layer)."""
        said = "this trainer was configured with"
        for option, what, prefix, keys, rows, geometry, extras in _PAGE_CHECKS:
            value = self.cfg.get(option, 0)
            tail = ": a checkpoint loads into the %s it was trained with only" % option
            have = [k for k in state_dict if isinstance(k, str) and k.startswith(prefix)]
            if value == 0:
                if have:
                    raise ValueError("%sout %s (%s=0), the state_dict holds %s%s" % (said, what, option, have[:2], tail))
                continue
            if any(k not in state_dict for k in keys):
                raise ValueError("%s %s=%d, the state_dict lacks %s%s"
                                 % (said, option, value, [k for k in keys if k not in state_dict], tail))
            w = state_dict[keys[0]]
            if torch.is_tensor(w) and (w.dim() != 2 or w.shape[0] != rows * value):
                raise ValueError("%s %s=%d, the state_dict's %s has shape %s (%s=%s)"
                                 % (said, option, value, keys[0], tuple(w.shape), option,
                                    w.shape[0] // rows if w.dim() == 2 else "?"))
            if extras is not None:
                extras(self.cfg, state_dict, said)
            if geometry is None:
                continue
            geo_option, heads_option, geo_keys = geometry
            geo, Hh = bool(self.cfg.get(geo_option, False)), self.cfg.get(heads_option, 1)
            for k in geo_keys(self.cfg):
                gw = state_dict.get(k)
                if geo != (gw is not None):
                    raise ValueError("%s %s=%r, the state_dict %s %s: a checkpoint loads into the %s it was trained with "
                                     "only" % (said, geo_option, geo, "lacks" if geo else "holds", k, geo_option))
                if geo and torch.is_tensor(gw) and tuple(gw.shape) != (Hh, 8):
                    raise ValueError("%s %s=True and %s=%d, the state_dict's %s has shape %s"
                                     % (said, geo_option, heads_option, Hh, k, tuple(gw.shape)))

    def _flat_buffers(self, spec):
        """Live BatchNorm buffers of an averaging trainer -> {key: view}: ``bbucket`` (float32, running_mean /
        running_var in state_dict order) and ``tracked`` (int64, one num_batches_tracked per BatchNorm)."""
        shapes = OrderedDict((k, s) for k, s in spec if k.endswith(("running_mean", "running_var")))
        counters = [k for k, _ in spec if k.endswith("num_batches_tracked")]
        self.bbucket = FlatBucket(shapes, self.device)
        self.tracked = torch.zeros(len(counters), dtype=torch.int64, device=self.device)
        views = dict(self.bbucket.views)
        views.update((k, self.tracked[i]) for i, k in enumerate(counters))
        return views

    def _setup_average(self):
        """The second flat bucket (and with ``average_buffers`` the second pair of buffer tensors), the device tables of
        the averaging launches and the start of the schedule.  Nothing is allocated when averaging is off."""
        self.n_averaged, self._avg_active = 0, False
        if self._avg is None:
            return
        self.abucket = self.pbucket.like()
        self._avg_buffers = self.buffers                    # average_buffers=False: the averaged model uses the live ones
        self.abbucket = self.atracked = None
        if self._avg.buffers:
            self.abbucket = self.bbucket.like()
            self.atracked = torch.zeros_like(self.tracked)
            counters = [k for k in self.buffers if k.endswith("num_batches_tracked")]
            views = dict(self.abbucket.views)
            views.update((k, self.atracked[i]) for i, k in enumerate(counters))
            self._avg_buffers = OrderedDict((k, views[k]) for k in self.buffers)
        self._stat_table = SegmentTable([(0, self.bbucket.flat.numel(), 0)], self.device)   # the running statistics
        # the device tensors, made here (no step copies a table to the device) and held only while the feature is on
        self._avg_seg, self._avg_bseg = self._run_table.args()[0], self._stat_table.args()[0]
        if self._avg.start == 0:
            self.reset_average()

    @property
    def average(self):
        """None when averaging is off; else the read-only record (kind, decay, warmup, start, every, buffers,
        n_averaged)."""
        return None if self._avg is None else self._avg._replace(n_averaged=self.n_averaged)

    def _need_average(self, what):
        if self._avg is None:
            raise RuntimeError("%s needs a trainer built with average=\"ema\" or \"swa\"" % what)

    def _not_averaged(self, what):
        if self._avg_active:
            raise RuntimeError("%s inside averaged_weights(): the trainer's views are the averaged model's" % what)

    def reset_average(self):
        """Restart the average from the current parameters and buffers (device copies): ``n_averaged`` 1 when the step
        count has reached ``average_start``, else 0 (the average then starts at that step)."""
        self._need_average("reset_average")
        self._not_averaged("reset_average")
        self.abucket.flat.copy_(self.pbucket.flat)
        if self._avg.buffers:
            self.abbucket.flat.copy_(self.bbucket.flat)
            self.atracked.copy_(self.tracked)
        self.n_averaged = 1 if self.update_count >= self._avg.start else 0

    def _average_step(self):
        """End of optimizer_step(): host integers decide, the device work is one launch per averaged flat buffer."""
        a, s = self._avg, self.update_count
        if s < a.start:
            return
        if self.n_averaged == 0:                            # step ``average_start``, or the first step after a resume past it
            self.reset_average()
            return
        if (s - a.start) % a.every:
            return
        w = average_weight(a.kind, a.decay, a.warmup, self.n_averaged)
        engine.call("cova_weight_average", self.abucket.flat, self.pbucket.flat, self.pbucket.flat.numel(),
                    *self._run_table.args(), w)
        if a.buffers:
            engine.call("cova_weight_average", self.abbucket.flat, self.bbucket.flat, self.bbucket.flat.numel(),
                        *self._stat_table.args(), w)
            self.atracked.copy_(self.tracked)               # copied, not averaged
        self.n_averaged += 1

    def averaged_state_dict(self):
        """The averaged model in the keys and layout of state_dict() (clones); with ``average_buffers=False`` its buffers
        are the live ones."""
        self._need_average("averaged_state_dict")
        if self.n_averaged == 0:
            raise RuntimeError("the average has not started (average_start=%d, step %d)" % (self._avg.start, self.update_count))
        sd = OrderedDict((k, v.detach().clone()) for k, v in self.abucket.views.items())
        sd.update((k, v.detach().clone()) for k, v in self._avg_buffers.items())
        return sd

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the block ``trainer.params`` (and with ``average_buffers`` ``trainer.buffers``) are the averaged
        views, so predict / evaluate / loss / evaluate_split / FeatureCache.check run on the averaged model with no copy;
        the live views are back on exit, also after an exception.  train_step, forward_backward, optimizer_step and
        load_state_dict raise RuntimeError inside it, as does entering it before the average has started."""
        self._need_average("averaged_weights")
        self._not_averaged("averaged_weights")
        if self.n_averaged == 0:
            raise RuntimeError("the average has not started (average_start=%d, step %d)" % (self._avg.start, self.update_count))
        live = self.params, self.buffers
        self.params, self.buffers, self._avg_active = self.abucket.views, self._avg_buffers, True
        try:
            yield self
        finally:
            (self.params, self.buffers), self._avg_active = live, False

    def _setup_accumulate(self):
        """The accumulator bucket and the device table of the trainable runs: neither with ``accumulate_steps=1``."""
        self.accumulated, self._update_count = 0, 0
        self._close = None                   # the closing micro-step's scale while its forward_backward runs
        if self.accumulate_steps == 1:
            return
        self.accbucket = self.pbucket.like()
        self._acc_seg = self._run_table.args()[0]            # made here if averaging has not: the same tensor

    @property
    def update_count(self):
        """Parameter updates made so far: what Adam's bias correction and the averaging schedule count.  With
        ``accumulate_steps=1`` it is ``step_count``."""
        return self._update_count if self.accumulate_steps > 1 else self.step_count

    def _no_pending(self, what):
        if self.accumulated:
            raise ValueError("%s with %d micro-batch(es) accumulated: finish the cycle with train_step() or make the "
                             "update with flush() first" % (what, self.accumulated))

    def _accumulate(self, mode, scale=1.0, lo=0, hi=None):
        """One cova_grad_accumulate launch over the trainable runs, cut to the flat range [lo, hi)."""
        n = self.gbucket.flat.numel()
        engine.call("cova_grad_accumulate", mode, self.accbucket.flat, self.gbucket.flat, n, *self._run_table.args(),
                    lo, n if hi is None else hi, scale)

    def flush(self):
        """Make the parameter update from the micro-batches pending (``accumulated`` = m >= 1, scale 1 / m with
        ``loss_reduction="mean"``): one closing cova_grad_accumulate launch, then optimizer_step()'s path.  -> whether an
        update happened; nothing is launched with none pending.  Under data parallelism a collective: every rank must
        hold the same ``accumulated``."""
        self._not_averaged("flush")
        if not self.accumulated:
            return False
        self._accumulate(ACC_CLOSE, accumulate_scale(self.loss_options["loss_reduction"], self.accumulated))
        self.accumulated = 0
        self._optimizer_step()
        return True

    def _average_tensors(self):
        """The tensors of the average that travel with broadcast_state / a broadcast optimizer state."""
        return [self.abucket.flat] + ([self.abbucket.flat, self.atracked] if self._avg.buffers else [])

    def _setup_finetune(self, frozen, bn_eval):
        for what, entries, names in (("frozen", frozen, list(self.params)),
                                     ("bn_eval", bn_eval, [k[:-len("running_mean")] for k in self.buffers
                                                           if k.endswith("running_mean")])):
            unknown = [e for e in entries if not any(_named_by(n, (e,)) for n in names)]
            if unknown:
                raise ValueError("%s names no %s: %s" % (what, "parameter" if what == "frozen" else "BatchNorm", unknown))
        self.frozen = frozenset(k for k in self.params if _named_by(k, frozen))
        eval_bns = [k[:-len("running_mean")] for k in self.buffers if k.endswith("running_mean")]
        eval_bns = [p for p in eval_bns if _named_by(p, bn_eval)]
        # (no entry: the bool of today's steps, exactly its launches)
        self.modes = {p: False for p in eval_bns} if eval_bns else True
        self.plan = (engine.grad_plan([k for k in self.params if k not in self.frozen],
                                      layer2=engine.has_layer2(self.params)) if self.frozen else None)
        # the runs of trainable tensors whatever their group (frozen ones are left out): cova_adam_step's slices, and
        # the one {lo, hi, 0, start} table that averaging and accumulation both launch over
        runs = group_runs(self.pbucket.offsets, self.pbucket.flat.numel(), self.frozen, dict.fromkeys(self.params, 0))
        self._adam_runs = [(lo, hi) for lo, hi, _ in runs]
        self._run_table = SegmentTable(runs, self.device)
        self.conv_frozen = all(k in self.frozen for k in self.params if k.startswith("convnet."))
        conv_bns = [k[:-len("running_mean")] for k in self.buffers if k.startswith("convnet.") and k.endswith("running_mean")]
        self.conv_bn_eval = all(not engine.is_train(self.modes, p) for p in conv_bns)

    def check_cached_features(self):
        """Cached RoI features stand for a conv stack that no step changes: every ``convnet.`` parameter frozen and every
        ``convnet.`` BatchNorm in eval mode (host flags, no device read)."""
        if not self.conv_frozen:
            raise ValueError("cached visual features need a frozen conv stack: build the trainer with "
                             "frozen=('convnet.',) (a trainable convnet. parameter would leave the cache stale)")
        if not self.conv_bn_eval:
            raise ValueError("cached visual features need the conv stack's BatchNorms in eval mode: build the trainer "
                             "with bn_eval=('convnet.',) (a train-mode BatchNorm normalises with batch statistics)")

    def _setup_optimizer(self, optimizer, momentum, dampening, nesterov, param_groups, max_grad_norm):
        """Resolve the parameter groups to merged runs of the flat bucket, once.  The default group (unclaimed trainable
        keys) is ``self.hp`` itself, so today's hyper-parameter dict, its checkpoint field and edits of it keep working."""
        self.optimizer = optimizer
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.hp.update(momentum=float(momentum), dampening=float(dampening), nesterov=bool(nesterov))
        claimed, groups = {}, []
        for i, spec in enumerate(param_groups or ()):
            if "params" not in spec:
                raise ValueError("param_groups[%d] has no 'params'" % i)
            extra = [k for k in spec if k != "params" and k not in _GROUP_HP]
            if extra:
                raise ValueError("param_groups[%d]: unknown option(s) %s (allowed: %s)" % (i, extra, _GROUP_HP))
            entries = _entries(spec["params"])
            unknown = [e for e in entries if not any(_named_by(k, (e,)) for k in self.params)]
            if unknown:
                raise ValueError("param_groups[%d] names no parameter: %s" % (i, unknown))
            keys = [k for k in self.params if _named_by(k, entries)]
            twice = [k for k in keys if k in claimed]
            if twice:
                raise ValueError("%s claimed by param_groups[%d] and [%d]" % (twice[:4], claimed[twice[0]], i))
            claimed.update((k, i) for k in keys)
            g = dict(params=[k for k in keys if k not in self.frozen], **{k: self.hp[k] for k in _GROUP_HP})
            g.update((k, v) for k, v in spec.items() if k != "params")
            groups.append(g)
        rest = [k for k in self.params if k not in self.frozen and k not in claimed]
        if rest or not groups:
            self.hp["params"] = rest
            groups.append(self.hp)
        if len(groups) > 16:
            raise ValueError("at most 16 parameter groups (cova_optim_step), got %d" % len(groups))
        for g in groups:
            g["betas"] = tuple(float(b) for b in g["betas"])
            g["nesterov"] = bool(g["nesterov"])
            _check_sgd_group(optimizer, g)
        self._groups = groups
        owner = {k: i for i, g in enumerate(groups) for k in g["params"]}
        self.optim_runs = group_runs(self.pbucket.offsets, self.pbucket.flat.numel(), self.frozen, owner)
        # no new option: optimizer_step() is today's cova_adam_step launch(es), the checkpoint format today's
        self._fused = optimizer != "adam" or param_groups is not None or self.max_grad_norm is not None
        self.momentum_buffer = torch.zeros_like(self.pbucket.flat) if optimizer == "sgd" else None
        self._buf_exists = [False] * len(groups)     # per group: torch creates the momentum buffer on its first step
        self.last_grad_norm = None
        self._norm_ws = None
        self._optim_table = SegmentTable(self.optim_runs, self.device)
        self._seg = self._optim_table.args()[0] if self._fused else None     # made here: no step copies it

    def _setup_criterion(self, class_weight, label_smoothing, focal_gamma, ignore_index, loss_reduction, track_metrics):
        """``class_weight`` becomes a device tensor that may be edited in place; the scalar options live in
        ``loss_options`` and are read (and checked) at every step: they travel as kernel arguments."""
        nc = int(self.cfg["n_classes"])
        engine.check_loss_options(nc, class_weight, label_smoothing, focal_gamma, ignore_index, loss_reduction)
        self.class_weight = (None if class_weight is None else
                             torch.as_tensor(class_weight).detach().to(torch.float32).to(self.device).contiguous().clone())
        self.loss_options = dict(label_smoothing=float(label_smoothing), focal_gamma=float(focal_gamma),
                                 ignore_index=None if ignore_index is None else int(ignore_index),
                                 loss_reduction=loss_reduction)
        self.metrics = LossMetrics(nc, self.device, self) if track_metrics else None
        self._loss_ws = None

    def _setup_mining(self, ratio, min_keep):
        """The mining options join ``loss_options`` only when a ratio is given (a default trainer's dict stays as it
        was); like the other scalar options they are read and checked at every step, so setting
        ``loss_options["hard_negative_ratio"]`` between steps turns mining on or off."""
        ratio, min_keep = engine.check_mining_options(ratio, min_keep)
        if ratio is not None:
            self.loss_options.update(hard_negative_ratio=ratio, hard_negative_min=min_keep)
        self.last_mined_labels = self.last_mining_counts = None

    def _mining(self):
        """None: mining is off; else this step's checked (ratio, min_keep)."""
        o = self.loss_options
        ratio, min_keep = engine.check_mining_options(o.get("hard_negative_ratio"), o.get("hard_negative_min", 0))
        return None if ratio is None else (ratio, min_keep)

    @staticmethod
    def _check_paged(batch, what):
        if batch.get("page_start") is None and batch.get("images") is None:
            raise ValueError("%s needs the batch's page_start (or its images, for the page count)" % what)

    @staticmethod
    def _page_start(batch, device):
        """The pages' row offsets (device int64 [B + 1]) without a host read: the batch's, or derived from the page
        column of the page-sorted bboxes and the page count of the images."""
        page_start = batch.get("page_start")
        if page_start is None:
            pages = torch.arange(int(batch["images"].shape[0]) + 1, dtype=torch.float32, device=device)
            page_start = torch.searchsorted(batch["bboxes"][:, 0].contiguous(), pages)
        return page_start.contiguous()

    def _mine(self, logits, batch, opts, mining):
        """cova_hard_negative_select on this step's logits -> (labels for the criterion, its options with the drop
        label as the ignore label).  No host read: page_start is the batch's, or comes from the page column of the
        page-sorted bboxes."""
        if opts["ignore_index"] is None:
            opts = dict(opts, ignore_index=engine.MINED_OUT)
        mined, _, counts = engine.hard_negative_select(logits, batch["labels"], self._page_start(batch, logits.device),
                                                       mining[0], mining[1], opts["ignore_index"], want_counts=True)
        self.last_mined_labels, self.last_mining_counts = mined, counts
        return mined, opts

    def _setup_rank(self, weight):
        """``page_rank_weight`` joins ``loss_options`` only when it is non-zero (a default trainer's dict stays as it
        was); it is read and checked at every step, so it may be set, changed or zeroed between steps."""
        weight = engine.check_rank_options(weight)
        if weight != 0.0:
            self.loss_options["page_rank_weight"] = weight
        self.last_rank_lists = self.last_rank_acc = None

    def _rank(self):
        """This step's checked weight of the ranking term; 0.0: the term is off."""
        return engine.check_rank_options(self.loss_options.get("page_rank_weight", 0.0))

    def _rank_term(self, logits, batch, rank_weight, loss, dl):
        """cova_page_rank_loss_fwd / _bwd on this step's logits: adds rank_weight * R to ``loss`` and its gradient to
        ``dl`` (None: the loss alone), the outputs of the cova_ce_loss pair -> (lists, acc).  The lists are read from the batch's own
        labels with the trainer's own ignore label, whatever mining relabelled for the cross-entropy."""
        o = self.loss_options
        ropts = dict(ignore_index=o["ignore_index"], reduction=o["loss_reduction"])
        page_start = self._page_start(batch, logits.device)
        lists, acc = engine.page_rank_loss_fwd(logits, batch["labels"], page_start, self.class_weight, ropts)
        if self.world_size > 1 and ropts["reduction"] == "mean":
            import torch.distributed as dist
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=self.group)
        engine.page_rank_loss_bwd(logits, batch["labels"], page_start, self.class_weight, ropts, lists, acc, rank_weight,
                                  into=(loss, dl))
        return lists, acc

    def _criterion(self):
        """None: the step's criterion is cova_ce_sum (no option set, no mining, no ranking term); else the checked
        options of this step."""
        o = self.loss_options
        if (self._mining() is None and self._rank() == 0.0 and self.class_weight is None and self.metrics is None and o["label_smoothing"] == 0.0
                and o["focal_gamma"] == 0.0 and o["ignore_index"] is None and o["loss_reduction"] == "sum"):
            return None
        return engine.check_loss_options(int(self.cfg["n_classes"]), None, o["label_smoothing"], o["focal_gamma"],
                                         o["ignore_index"], o["loss_reduction"])

    @property
    def loss_path(self):
        """The entry point(s) the next step's criterion runs through: "cova_ce_sum" or "cova_ce_loss"."""
        return "cova_ce_sum" if self._criterion() is None else "cova_ce_loss"

    def _criterion_fwd_bwd(self, logits, labels, opts, metrics, want_grad=True):
        """cova_ce_loss_fwd, the all-reduce of its three float64 sums where the mean is over the global batch, and
        cova_ce_loss_bwd -> (loss [1], dlogits, pred)."""
        n_ws = engine.query("cova_ce_loss_workspace_doubles", logits.shape[0])
        if self._loss_ws is None or self._loss_ws.numel() < n_ws:
            self._loss_ws = torch.empty(n_ws, dtype=torch.float64, device=self.device)
        acc, pred = engine.ce_loss_fwd(logits, labels, self.class_weight, opts, metrics, workspace=self._loss_ws)
        if self.world_size > 1 and opts["reduction"] == "mean":
            import torch.distributed as dist
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=self.group)
        loss, dl = engine.ce_loss_bwd(logits, labels, self.class_weight, opts, acc, want_grad=want_grad)
        return loss, dl, pred

    @property
    def param_groups(self):
        """The live parameter groups ({"params": [keys], lr, weight_decay, betas, eps, momentum, dampening, nesterov}): a
        hyper-parameter edited between steps (a manual schedule) applies at the next optimizer_step().  Membership is
        fixed at construction."""
        return self._groups

    def broadcast_state(self, src=0):
        """Rank `src`'s parameters, BatchNorm buffers, Adam moments and step count to every rank: replicas start (and
        resume) from ONE state even when the ranks were built from rank-local checkpoints."""
        import torch.distributed as dist
        self._not_averaged("broadcast_state")
        self._no_pending("broadcast_state")
        extra = [self.momentum_buffer] if self.momentum_buffer is not None else []
        if self._avg is not None:
            extra = extra + [t for t in self._average_tensors() if t.numel()]
        for t in [self.pbucket.flat, self.exp_avg, self.exp_avg_sq] + extra + [self.buffers[k] for k in sorted(self.buffers)]:
            dist.broadcast(t, src=src, group=self.group)
        flags = [int(b) for b in self._buf_exists] if self.momentum_buffer is not None else []
        counter = [self.n_averaged] if self._avg is not None else []
        updates = [self._update_count] if self.accumulate_steps > 1 else []
        step = torch.tensor(updates + [self.step_count] + flags + counter, dtype=torch.int64, device=self.device)
        dist.broadcast(step, src=src, group=self.group)
        got = step.tolist()
        if updates:
            self._update_count = int(got.pop(0))
        self.step_count = int(got[0])
        self._buf_exists = [bool(b) for b in got[1:1 + len(flags)]] if flags else self._buf_exists
        if counter:
            self.n_averaged = int(got[-1])

    def exposed_allreduce_ms(self):
        """Mean time per step the stream spent in optimizer_step's gradient collectives (HIP events on the compute
        stream around the all-reduce calls / waits: what the overlap did not hide); 0 on a single rank."""
        if not self._ar_events:
            return 0.0
        torch.cuda.synchronize(self.device)
        ms = sum(a.elapsed_time(b) for a, b in self._ar_events) / len(self._ar_events)
        self._ar_events = []
        return ms

    def state_dict(self):
        sd = OrderedDict()
        for k in list(self.params) + list(self.buffers):
            sd[k] = (self.params[k] if k in self.params else self.buffers[k]).detach().clone()
        return sd

    def _all_ranks_ok(self, ok, what):
        """Collective: every rank learns whether ALL ranks validated `what`; raises the same error everywhere instead of
        leaving the ranks that did validate blocked in the broadcast that follows."""
        import torch.distributed as dist
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
        if int(flag.item()) == 0:
            raise KeyError("%s: at least one rank could not validate its argument (this rank: %s)" % (what, "ok" if ok else "failed"))

    def load_state_dict(self, state_dict, broadcast=False):
        """Restore parameters and BatchNorm buffers from a reference-layout state_dict -- the save-best /
        reload-best cycle of train.py:84,94 (`torch.save(model.state_dict())`, `load_state_dict(torch.load(...))`).
        The flat buffers keep their addresses (views, moments and bucket stay valid).

        Local by default: a rank-0-only reload ("reload best, evaluate on rank 0") involves no collective.  With
        `broadcast=True` the call IS a collective that EVERY rank must make: the keys are validated on all ranks first
        (one all-reduce of an ok flag, so a KeyError on one rank raises on all of them), then rank 0's parameters and
        buffers -- what was loaded, not the Adam moments or the step count -- replace every rank's.

        With ``average=`` the average restarts from what was loaded, as reset_average() does; to resume an average,
        load the state dict first and the optimizer state (which carries the average) after it."""
        self._not_averaged("load_state_dict")
        self._check_page_layers(state_dict)
        missing = [k for k in list(self.params) + list(self.buffers) if k not in state_dict]
        # sizes are part of the validation every rank agrees on BEFORE any copy / broadcast: a tensor of the wrong size on
        # one rank raising inside copy_ would leave the other ranks blocked in dist.broadcast
        bad = [k for k in list(self.params) + list(self.buffers)
               if k in state_dict and (not torch.is_tensor(state_dict[k]) or
                                       state_dict[k].numel() != (self.params[k] if k in self.params else self.buffers[k]).numel())]
        if broadcast and self.world_size > 1:
            self._all_ranks_ok(not missing and not bad, "load_state_dict")
        if missing:
            raise KeyError("state_dict lacks %s" % missing[:4])
        if bad:
            self._check_attention_mode(state_dict)
            raise ValueError("state_dict entries of the wrong size: %s" % bad[:4])
        for k, p in self.params.items():
            p.copy_(state_dict[k].to(p.device).view_as(p))
        for k in self.buffers:
            self.buffers[k].copy_(state_dict[k].to(self.device).view_as(self.buffers[k]))
        if broadcast and self.world_size > 1:
            import torch.distributed as dist
            for t in [self.pbucket.flat] + [self.buffers[k] for k in sorted(self.buffers)]:
                dist.broadcast(t, src=0, group=self.group)
        self.accumulated = 0                 # pending micro-batches belonged to the parameters just replaced
        if self._avg is not None:
            self.reset_average()

    def optimizer_state_dict(self):
        """Adam moments + step count (the reference keeps no optimizer state in its checkpoints, train.py:84;
        with this a run can be resumed exactly).  With ``accumulate_steps`` > 1 also "updates", the parameter updates;
        it is taken at a cycle boundary (ValueError while micro-batches are pending)."""
        self._no_pending("optimizer_state_dict")
        st = dict(step=self.step_count, exp_avg=self.exp_avg.detach().clone(),
                  exp_avg_sq=self.exp_avg_sq.detach().clone(), hp={k: self.hp[k] for k in _ADAM_HP})
        if self._fused:     # (with no new option the format stays today's: an Adam checkpoint has no "algorithm")
            st.update(algorithm=self.optimizer,
                      groups=[dict(params=list(g["params"]), **{k: g[k] for k in _GROUP_HP}) for g in self._groups],
                      momentum_buffer=None if self.momentum_buffer is None else self.momentum_buffer.detach().clone(),
                      momentum_buffer_exists=list(self._buf_exists))
        if self.accumulate_steps > 1:
            st["updates"] = self.update_count
        if self._avg is not None:
            st["average"] = dict(self.average._asdict(), flat=self.abucket.flat.detach().clone(),
                                 buffers_flat=self.abbucket.flat.detach().clone() if self._avg.buffers else None,
                                 num_batches_tracked=self.atracked.detach().clone() if self._avg.buffers else None)
        return st

    def _check_optimizer_state(self, state):
        """(what is wrong with `state` beyond the Adam fields, or None) -- a checkpoint without "algorithm" is Adam's."""
        updates = state.get("updates")
        if self.accumulate_steps == 1 and updates is not None and int(updates) != int(state.get("step", updates)):
            return ("optimizer state of %d parameter updates in %d steps: it was written with accumulate_steps > 1 and "
                    "loads into a trainer built with accumulate_steps > 1 only" % (int(updates), int(state["step"])))
        algorithm = state.get("algorithm", "adam")
        if algorithm != self.optimizer:
            return "optimizer state of algorithm %r, this trainer runs %r" % (algorithm, self.optimizer)
        groups = state.get("groups")
        if groups is not None and [list(g.get("params", ())) for g in groups] != [g["params"] for g in self._groups]:
            return "optimizer state with other parameter groups (%d groups)" % len(groups)
        buf = state.get("momentum_buffer")
        if buf is not None and not (torch.is_tensor(buf) and buf.numel() == self.pbucket.flat.numel()):
            return "momentum buffer of the wrong size (expected %d elements)" % self.pbucket.flat.numel()
        if len(state.get("momentum_buffer_exists", self._buf_exists)) != len(self._groups):
            return "momentum_buffer_exists does not have one flag per group"
        avg = state.get("average")
        if avg is not None and self._avg is not None:       # (a trainer without averaging ignores the entry)
            if avg.get("kind") != self._avg.kind:
                return "average of kind %r, this trainer keeps %r" % (avg.get("kind"), self._avg.kind)
            want = [("flat", self.abucket.flat)]
            if self._avg.buffers:
                want += [("buffers_flat", self.abbucket.flat), ("num_batches_tracked", self.atracked)]
            for k, t in want:
                if not (torch.is_tensor(avg.get(k)) and avg[k].numel() == t.numel()):
                    return "average: %r of the wrong size (expected %d elements)" % (k, t.numel())
            if int(avg.get("n_averaged", -1)) < 0:
                return "average without n_averaged"
        return None

    def load_optimizer_state_dict(self, state, broadcast=False):
        """Moments (Adam) or momentum buffer (SGD), step count and hyper-parameters.  Local by default; `broadcast=True`
        makes it a collective every rank must call (validated on all ranks first) after which every rank holds rank 0's
        moments, step count and hyper-parameters.  A state of another algorithm raises (on every rank when broadcasting).

        With ``average=``: an "average" entry of this trainer's kind and size restores the average and ``n_averaged``
        (another kind or size raises ValueError like another algorithm); without the entry the average stays as
        load_state_dict() left it.  The averaging options stay the constructor's."""
        self._not_averaged("load_optimizer_state_dict")
        ok = all(k in state for k in ("step", "exp_avg", "exp_avg_sq"))
        sized = ok and all(torch.is_tensor(state[k]) and state[k].numel() == self.exp_avg.numel() for k in ("exp_avg", "exp_avg_sq"))
        problem = self._check_optimizer_state(state)
        if broadcast and self.world_size > 1:
            self._all_ranks_ok(ok and sized and problem is None, "load_optimizer_state_dict")   # (sizes too: see load_state_dict)
        if not ok:
            raise KeyError("optimizer state lacks one of step / exp_avg / exp_avg_sq")
        if not sized:
            raise ValueError("optimizer state moments of the wrong size (expected %d elements)" % self.exp_avg.numel())
        if problem is not None:
            raise ValueError(problem)
        self.step_count = int(state["step"])
        self._update_count = int(state.get("updates", self.step_count))
        self.accumulated = 0
        self.exp_avg.copy_(state["exp_avg"].to(self.device).view_as(self.exp_avg))
        self.exp_avg_sq.copy_(state["exp_avg_sq"].to(self.device).view_as(self.exp_avg_sq))
        self.hp.update(state.get("hp", {}))
        for g, s in zip(self._groups, state.get("groups") or ()):
            g.update((k, s[k]) for k in _GROUP_HP if k in s)
        if self.momentum_buffer is not None:
            buf = state.get("momentum_buffer")
            if buf is not None:
                self.momentum_buffer.copy_(buf.to(self.device).view_as(self.momentum_buffer))
            else:
                self.momentum_buffer.zero_()
            self._buf_exists = [bool(b) for b in state.get("momentum_buffer_exists", [False] * len(self._groups))]
        avg = state.get("average") if self._avg is not None else None
        if avg is not None:
            self.abucket.flat.copy_(avg["flat"].to(self.device).view_as(self.abucket.flat))
            if self._avg.buffers:
                self.abbucket.flat.copy_(avg["buffers_flat"].to(self.device).view_as(self.abbucket.flat))
                self.atracked.copy_(avg["num_batches_tracked"].to(self.device).view_as(self.atracked))
            self.n_averaged = int(avg["n_averaged"])
        if broadcast and self.world_size > 1:
            import torch.distributed as dist
            for t in (self.exp_avg, self.exp_avg_sq):
                dist.broadcast(t, src=0, group=self.group)
            if self._avg is not None:
                for t in self._average_tensors():
                    if t.numel():
                        dist.broadcast(t, src=0, group=self.group)
                counter = torch.tensor([self.n_averaged], dtype=torch.int64, device=self.device)
                dist.broadcast(counter, src=0, group=self.group)
                self.n_averaged = int(counter.item())
            b1, b2 = self.hp["betas"]
            updates = [float(self._update_count)] if self.accumulate_steps > 1 else []
            meta = torch.tensor([float(self.step_count), self.hp["lr"], self.hp["weight_decay"], b1, b2, self.hp["eps"]]
                                + updates, dtype=torch.float64, device=self.device)
            dist.broadcast(meta, src=0, group=self.group)
            m = meta.tolist()
            self.step_count = int(m[0])
            if updates:
                self._update_count = int(m[6])
            self.hp.update(lr=m[1], weight_decay=m[2], betas=(m[3], m[4]), eps=m[5])
            if self._fused:
                self._broadcast_groups()

    def _broadcast_groups(self):
        """Rank 0's per-group hyper-parameters, momentum buffer and its per-group flags to every rank."""
        import torch.distributed as dist
        meta = torch.tensor(group_rows(self._groups, self._buf_exists), dtype=torch.float64, device=self.device)
        dist.broadcast(meta, src=0, group=self.group)
        for g, r in zip(self._groups, meta.tolist()):
            g.update(lr=r[0], weight_decay=r[1], betas=(r[2], r[3]), eps=r[4], momentum=r[5], dampening=r[6],
                     nesterov=bool(r[7]))
        self._buf_exists = [bool(r[8]) for r in meta.tolist()]
        if self.momentum_buffer is not None:
            dist.broadcast(self.momentum_buffer, src=0, group=self.group)

    def forward_backward(self, batch, masks=None):
        """Forward + criterion + backward into the flat gradient bucket.  Returns (loss, pred): the local CE sum, or
        with criterion options the local sum ("sum") / the mean over the global batch ("mean").  A batch with
        ``visual_feats`` (DeviceDataset.batches(features=)) skips the conv stack and the RoI op; it raises ValueError
        unless the conv stack is frozen with its BatchNorms in eval mode."""
        self._not_averaged("forward_backward")
        opts, mining, rank_weight = self._criterion(), self._mining(), self._rank()
        if mining is not None:
            self._check_paged(batch, "hard-negative mining")
        if rank_weight != 0.0:
            self._check_paged(batch, "the page ranking loss")
        # With SyncBN a one-box shard is legal (the statistics are over the whole batch, as torch.nn.SyncBatchNorm
        # accepts it): the train-mode "more than 1 value per channel" check then applies to the GLOBAL box count, which
        # _stat_sync has from its all-reduce -- every rank raises together instead of one rank leaving the others
        # blocked in a collective.
        vis = batch.get("visual_feats")
        if vis is not None:
            self.check_cached_features()
        engine.check_batch(self.cfg, batch.get("images"), batch["bboxes"], batch["additional_feats"],
                           batch["context_indices"], self.modes if not self.sync_bn else False, vis)
        self.step_count += 1
        base = (self.dropout_seed * 0x9E3779B1 + 2 * self.step_count) & 0xFFFFFFFFFFFF
        if self.sync_bn:
            engine.STAT_SYNC = self._stat_sync(batch)
        try:
            logits, sv = engine.model_fwd(self.cfg, self.params, self.buffers, batch.get("images"),
                                          batch["bboxes"], batch["additional_feats"],
                                          batch["context_indices"], self.modes, (base, base + 1), masks,
                                          plan=self.plan, visual_feats=vis, page_size=batch.get("page_size"),
                                          page_start=batch.get("page_start"))
            if opts is None:
                loss, dl, pred = engine.ce_sum(logits, batch["labels"])
            else:
                labels = batch["labels"]
                if mining is not None:
                    labels, opts = self._mine(logits, batch, opts, mining)
                loss, dl, pred = self._criterion_fwd_bwd(logits, labels, opts,
                                                         None if self.metrics is None else self.metrics.buf)
                if rank_weight != 0.0:
                    self.last_rank_lists, self.last_rank_acc = self._rank_term(logits, batch, rank_weight, loss, dl)
            self._head_work = None
            # (an accumulating trainer exchanges gradients on the closing micro-step of train_step() only)
            overlap = (self.world_size > 1 and engine.OPTIONS.overlap_allreduce
                       and (self.accumulate_steps == 1 or self._close is not None))
            engine.model_bwd(sv, dl, self.params, self.grads,
                             after_head=self._reduce_head if overlap else None, plan=self.plan)
        finally:
            engine.STAT_SYNC = None
        return loss, pred

    def _stat_sync(self, batch):
        """SyncBN bookkeeping of one step: whole-batch / local element-count ratios for the page-shaped
        (conv stack) and box-shaped (BatchNorm1d) statistics; one tiny all-reduce + host read."""
        import torch.distributed as dist
        images = batch.get("images")                                                           # host ints: no device read
        n_pages = int(images.shape[0]) if images is not None else int(batch["page_start"].shape[0]) - 1
        n_boxes = int(batch["bboxes"].shape[0])
        total = torch.tensor([n_pages, n_boxes], dtype=torch.float64, device=self.device)
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)
        tot = total.tolist()                                                                   # the step's one host read
        r = [tot[0] / max(float(n_pages), 1.0), tot[1] / max(float(n_boxes), 1.0)]
        if tot[1] == 1.0:
            raise ValueError("Expected more than 1 value per channel when training (1 box in the whole batch)")
        return engine.StatSync(self.group, r[0], r[1])

    # Gradient exchange: the head (positional encoder, GAT, decoder = 96 % of the 6.5 MB bucket, the
    # tail of the flat buffer) is complete before the conv-stack backward starts, so its all-reduce is
    # issued there and runs over xGMI under ~6 ms of convolutions; only the 0.6 MB conv-stack part
    # is exchanged at the end of the step.
    def _head_offset(self):
        for k in self.gbucket.offsets:               # state_dict order: conv stack first
            if not k.startswith("convnet."):
                return self.gbucket.split_at(k)
        return self.gbucket.flat.numel()

    def _reduce_head(self):
        lo = self._head_offset()
        if lo >= self.gbucket.flat.numel():
            return
        if self._close is not None:          # the head part of the cycle closes here, the conv part after model_bwd
            self._accumulate(ACC_ADD_CLOSE, self._close, lo, self.gbucket.flat.numel())
        self._head_work = self.gbucket.all_reduce_range(lo, self.gbucket.flat.numel(), self.group,
                                                        async_op=True)

    def optimizer_step(self):
        self._not_averaged("optimizer_step")
        self._no_pending("optimizer_step")
        self._optimizer_step()

    def _optimizer_step(self):
        if self.accumulate_steps > 1:
            self._update_count += 1
        self._update_parameters()
        if self._avg is not None:
            self._average_step()

    def _update_parameters(self):
        if self.world_size > 1:
            timing = self.measure_allreduce and len(self._ar_events) < 4096
            if timing:                      # events on THIS trainer's device / stream (not the process' current device)
                st = torch.cuda.current_stream(self.device)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
            if getattr(self, "_head_work", None) is not None:
                if not self.conv_frozen:            # (a frozen conv stack has no gradients to exchange)
                    self.gbucket.all_reduce_range(0, self._head_offset(), self.group)
                self._head_work.wait()
                self._head_work = None
            elif self.conv_frozen:
                lo = self._head_offset()
                if lo < self.gbucket.flat.numel():
                    self.gbucket.all_reduce_range(lo, self.gbucket.flat.numel(), self.group)
            else:
                self.gbucket.all_reduce_sum(self.group)
            if timing:
                e1.record(st)
                self._ar_events.append((e0, e1))
        if self._fused:
            self._fused_step()
            return
        b1, b2 = self.hp["betas"]
        if not self.frozen:
            engine.call("cova_adam_step", self.pbucket.flat, self.gbucket.flat, self.exp_avg,
                        self.exp_avg_sq, self.pbucket.flat.numel(), self.update_count, self.hp["lr"], b1, b2,
                        self.hp["eps"], self.hp["weight_decay"])
            return
        for lo, hi in self._adam_runs:          # frozen tensors: parameters and moments untouched
            engine.call("cova_adam_step", self.pbucket.flat[lo:hi], self.gbucket.flat[lo:hi], self.exp_avg[lo:hi],
                        self.exp_avg_sq[lo:hi], hi - lo, self.update_count, self.hp["lr"], b1, b2,
                        self.hp["eps"], self.hp["weight_decay"])

    def _fused_step(self):
        """Clip (optional) and update every group in one cova_optim_step launch.  Under DDP this runs after both phases
        of the all-reduce, so every rank takes the norm of the same reduced gradients and clips identically; the clip
        coefficient stays on the device and scales g as the kernel loads it, so the gradient bucket keeps the unclipped
        reduced gradients and no host read happens."""
        flat, n = self.pbucket.flat, self.pbucket.flat.numel()
        gscale = None
        if self.max_grad_norm is not None:
            if self._norm_ws is None:
                n_ws = engine.query("cova_grad_norm_workspace_doubles", self._optim_table.total)
                self._norm_ws = torch.empty(n_ws, dtype=torch.float64, device=self.device)
            out = torch.empty(2, dtype=torch.float32, device=self.device)        # [norm, clip coefficient]
            engine.call("cova_grad_norm", self.gbucket.flat, n, *self._optim_table.args(), self.max_grad_norm,
                        self._norm_ws, out)
            self.last_grad_norm, gscale = out[0], out[1:]
        if not self.optim_runs:
            return
        # host table [groups][9], read by the launch itself (kernel arguments)
        table = torch.tensor(group_rows(self._groups, self._buf_exists), dtype=torch.float64)
        sgd = self.optimizer == "sgd"
        engine.call("cova_optim_step", OPTIMIZERS.index(self.optimizer), flat, self.gbucket.flat,
                    self.momentum_buffer if sgd else self.exp_avg, None if sgd else self.exp_avg_sq, n,
                    *self._optim_table.args(), table.data_ptr(), len(self._groups), self.update_count, gscale)
        if sgd:
            self._buf_exists = [b or g["momentum"] != 0 for g, b in zip(self._groups, self._buf_exists)]

    def train_step(self, batch, masks=None):
        """optimizer.zero_grad(); forward; loss; backward; optimizer.step()  (train.py:45-60).
        Gradients are fully overwritten each step, so zero_grad is implicit.

        With ``accumulate_steps`` n > 1 this is one micro-step: forward and backward, then one cova_grad_accumulate launch
        that opens (first micro-step of a cycle) or adds to the accumulator; the n-th closes the cycle into the gradient
        bucket (scale 1 / n with ``loss_reduction="mean"``) and makes the update.  Only that one exchanges gradients
        between ranks.  Returns the micro-batch's (loss, pred)."""
        self._not_averaged("train_step")
        if self.accumulate_steps == 1:
            loss, pred = self.forward_backward(batch, masks)
            self.optimizer_step()
            return loss, pred
        m = self.accumulated + 1
        if m < self.accumulate_steps:
            loss, pred = self.forward_backward(batch, masks)
            self._accumulate(ACC_OPEN if m == 1 else ACC_ADD)
            self.accumulated = m
            return loss, pred
        self._close = accumulate_scale(self.loss_options["loss_reduction"], m)
        try:
            loss, pred = self.forward_backward(batch, masks)
            if self._head_work is None:
                self._accumulate(ACC_ADD_CLOSE, self._close)
            elif not self.conv_frozen:       # the head part was closed before its all-reduce started (_reduce_head)
                self._accumulate(ACC_ADD_CLOSE, self._close, 0, self._head_offset())
        finally:
            self._close = None
        self.accumulated = 0
        self._optimizer_step()
        return loss, pred

    @torch.no_grad()
    def evaluate(self, batch, page_start, k=1, decode="column", score="map"):
        """Eval-mode decisions of train.py:131-154 for one batch.  ``page_start`` int64 [n_pages+1]
        box offsets.  Returns (topk [n_pages, n_classes, k] page-local box indices, best first;
        correct [n_pages, n_classes-1] bool = the labelled box of class c is among the top k).
        ``decode="joint"`` (k must be 1, at most 7 classes, else ValueError): ``topk[:, 1:, 0]`` is the joint choice of
        cova_page_joint_decode -- one distinct box per class, scored by ``score`` ("map": logit minus the background
        logit, "logit") -- and ``correct`` its hit table (== 1); column 0 stays the arg-max of the background column."""
        mode = engine.check_decode(decode, score, int(self.cfg["n_classes"]), k)
        logits, _ = self.predict(batch)
        n_pages, nc = page_start.numel() - 1, logits.shape[1]
        topk = torch.empty((n_pages, nc, k), dtype=torch.int64, device=logits.device)
        engine.call("cova_page_class_topk", logits, page_start.contiguous(), n_pages, nc, k, topk)
        if decode == "joint":
            tab = torch.full((2, n_pages, nc - 1), -2, dtype=torch.int32, device=logits.device)
            engine.call("cova_page_joint_decode", logits, batch["labels"], page_start.contiguous(), None, n_pages, nc,
                        n_pages, mode, tab[0], tab[1], None)
            topk[:, 1:, 0] = tab[0]
            return topk, tab[1] == 1
        # train.py:146: the labelled box of class c is the FIRST box of that class within the page;
        # a page without one scores False (the reference would raise an IndexError there)
        labels = batch["labels"]
        n_boxes = labels.numel()
        page_of = torch.searchsorted(page_start[1:].contiguous(), torch.arange(n_boxes, device=labels.device),
                                     right=True)
        local = torch.arange(n_boxes, device=labels.device) - page_start[page_of]
        correct = []
        for c in range(1, nc):
            first = torch.full((n_pages,), n_boxes, dtype=torch.int64, device=labels.device)
            sel = labels == c
            first.scatter_reduce_(0, page_of[sel], local[sel], reduce="amin")
            has = first < n_boxes
            correct.append(has & (topk[:, c, :] == first.view(-1, 1)).any(dim=1))
        return topk, torch.stack(correct, dim=1)

    @torch.no_grad()
    def predict(self, batch):
        """Eval-mode forward (running statistics) -> (logits, per-box argmax).  A batch with ``visual_feats`` (cached RoI
        features, features.FeatureCache) needs no images: the rows come from the table."""
        vis = batch.get("visual_feats")
        engine.check_batch(self.cfg, batch.get("images"), batch["bboxes"], batch["additional_feats"],
                           batch["context_indices"], False, vis)
        logits, _ = engine.model_fwd(self.cfg, self.params, self.buffers, batch.get("images"),
                                     batch["bboxes"], batch["additional_feats"],
                                     batch["context_indices"], False, save=False, visual_feats=vis,
                                     page_size=batch.get("page_size"), page_start=batch.get("page_start"))
        _, _, pred = engine.ce_sum(logits, None, want_grad=False)
        return logits, pred

    @torch.no_grad()
    def loss(self, batch):
        """Validation loss: eval-mode forward (running statistics, as predict) and the configured criterion (without
        options CrossEntropyLoss(reduction="sum")), the page ranking term included when ``page_rank_weight`` is set.
        Returns the device scalar; ``metrics`` is not touched."""
        rank_weight = self._rank()
        if rank_weight != 0.0:
            self._check_paged(batch, "the page ranking loss")
        logits, _ = self.predict(batch)
        opts = self._criterion() or engine.check_loss_options(int(self.cfg["n_classes"]))
        loss, _, _ = self._criterion_fwd_bwd(logits, batch["labels"], opts, None, want_grad=False)
        if rank_weight != 0.0:
            self._rank_term(logits, batch, rank_weight, loss, None)
        return loss[0]
