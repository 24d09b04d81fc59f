"""Cached RoI visual features for head-only training and evaluation on a frozen backbone.

With ``HotPathTrainer(frozen=("convnet.",), bn_eval=("convnet.",))`` the conv stack's parameters and BatchNorm buffers
never change and its BatchNorms normalise with running statistics, so the RoI-pooled visual row of a box is a function
of its page, its coordinates and constants.  ``FeatureCache.build`` computes that row once for every box of a
``pipeline.DeviceDataset`` into a split-resident table [R, n_vis] (R = boxes of the split, row r = box r of
``dataset.rows``), with the very launches a frozen step and ``predict`` issue.  ``DeviceDataset.batches(features=cache)``
then yields batches without images that carry ``visual_feats = (table, row_ids)``; the model's forward turns them into
``comb[:, :n_vis]`` with one cova_feat_rows_gather launch (engine.model_fwd): no page gather, no conv stack, no RoI op.

A cache is only valid for the conv stack and the split it was built from.  The *stamp* records both: a device copy of
every ``convnet.`` parameter and buffer, the configuration fields that shape the rows, the split's ``P, H, W``, its
per-page box counts and its box coordinates.  ``check`` compares the stamp with a trainer and a dataset (one device
comparison, one host read; call it outside step loops -- ``evaluation.evaluate_split`` and ``evaluation.fit`` do, once
on entry).  ``save`` / ``load`` keep table and stamp together, so the jobs of a sweep can share one build.

Under data parallelism every rank builds (or loads) the whole table: the shuffled shards change every epoch.
"""
import numpy as np
import torch

from . import engine
from .pipeline import epoch_plan

# the configuration fields that shape a visual row, with the defaults engine.model_fwd applies
CFG_FIELDS = (("backbone", "resnet18"), ("backbone_layers", 1), ("roi_output_size", None), ("roi_op", "pool"),
              ("sampling_ratio", 2), ("roi_aligned", False), ("spatial_scale", None))
FORMAT = 1


def stamp_cfg(cfg):
    """The row-shaping fields of ``cfg`` as plain values (defaults filled in)."""
    out = {}
    for k, default in CFG_FIELDS:
        v = cfg.get(k, default)
        if k == "roi_output_size":
            v = tuple(int(x) for x in v)
        elif k == "spatial_scale":
            v = None if not v else float(v)           # (falsy: derived from the feature map, as model_fwd does)
        elif k == "roi_aligned":
            v = bool(v)
        elif k in ("backbone_layers", "sampling_ratio"):
            v = int(v)
        out[k] = v
    return out


def _dev(d):
    """torch.device with the index filled in ("cuda" is the current device)."""
    d = torch.device(d)
    return torch.device(d.type, torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def conv_keys(trainer):
    """The ``convnet.`` state_dict keys of a trainer (parameters and BatchNorm buffers), sorted."""
    return sorted(k for k in list(trainer.params) + list(trainer.buffers) if k.startswith("convnet."))


def _tensor_of(trainer, k):
    return trainer.params[k] if k in trainer.params else trainer.buffers[k]


def _bits(t):
    """A tensor's bytes as a flat int32 vector (float32 and int64 tensors): equality of bits, NaNs included."""
    return t.detach().contiguous().reshape(-1).view(torch.int32)


def conv_bits(trainer, keys):
    """Every ``convnet.`` tensor of the trainer back to back, as bits: what a stamp is compared with."""
    return torch.cat([_bits(_tensor_of(trainer, k)) for k in keys])


class FeatureCache:
    """``table`` float32 [R, n_vis] on the device and the stamp of what it was computed from (module docstring)."""

    def __init__(self, table, stamp):
        self.table, self.stamp = table, stamp

    # ------------------------------------------------------------------------------------------------ properties
    @property
    def device(self):
        return self.table.device

    @property
    def n_vis(self):
        return int(self.table.shape[1])

    @property
    def nbytes(self):
        """Size of the table in bytes (the stamp adds the conv stack's 0.6 MB at ResNet-18 and 16 bytes per box)."""
        return int(self.table.numel()) * self.table.element_size()

    def __len__(self):
        return int(self.table.shape[0])

    # ------------------------------------------------------------------------------------------------ build
    @classmethod
    @torch.no_grad()
    def build(cls, trainer, dataset, batch_size=10, prefetch=True):
        """One eval-mode pass of the conv stack and the RoI op over ``dataset`` in dataset order, nothing sampled: the
        launches of ``trainer.predict`` up to the RoI output, which is pointed at the table slice of the batch's boxes
        (leading dimension n_vis) -- no gather, no copy, no host read inside the loop."""
        trainer.check_cached_features()
        cfg, dev = trainer.cfg, trainer.device
        if _dev(dataset.device) != _dev(dev):
            raise ValueError("FeatureCache.build: the dataset lives on %s, the trainer on %s" % (dataset.device, dev))
        if int(batch_size) < 1:
            raise ValueError("FeatureCache.build: batch_size must be >= 1")
        n_vis = engine.backbone_feat(cfg)
        R = int(dataset.starts[-1])
        table = torch.empty((R, n_vis), dtype=torch.float32, device=dev)
        align = cfg.get("roi_op", "pool") == "align"
        roi_size = tuple(cfg["roi_output_size"])
        plan = epoch_plan(dataset.P, int(batch_size), False, 0, 0)
        for ids, batch in zip(plan, dataset.batches(int(batch_size), prefetch=prefetch)):
            # host ints: the pages of a batch are consecutive and every box is kept, so the batch's boxes are the rows
            # starts[first page] .. starts[last page + 1] of the table
            first, n = int(dataset.starts[ids[0]]), int(batch["bboxes"].shape[0])
            assert n == int(dataset.starts[ids[-1] + 1]) - first
            if n == 0:
                continue
            out = table[first:first + n]
            images = batch["images"]
            feat, _ = engine.convstack_fwd(images, trainer.params, trainer.buffers, False, save=False,
                                           lazy_out=not align)
            scale = cfg.get("spatial_scale") or feat.shape[1] / images.shape[2]
            if align:
                engine.roialign_fwd(feat, batch["bboxes"], roi_size, scale, cfg.get("sampling_ratio", 2),
                                    cfg.get("roi_aligned", False), out, n_vis)
            else:
                engine.roipool_fwd(feat, batch["bboxes"], roi_size, scale, out, n_vis)
        return cls(table, cls.make_stamp(trainer, dataset))

    @staticmethod
    def make_stamp(trainer, dataset):
        keys = conv_keys(trainer)
        return dict(format=FORMAT, cfg=stamp_cfg(trainer.cfg), P=int(dataset.P), H=int(dataset.H), W=int(dataset.W),
                    counts=torch.from_numpy(np.asarray(dataset.counts, dtype=np.int64).copy()),
                    keys=keys, shapes=[tuple(_tensor_of(trainer, k).shape) for k in keys],
                    conv=conv_bits(trainer, keys).clone(), boxes=dataset.rows[:, :4].contiguous().clone())

    # ------------------------------------------------------------------------------------------------ checks
    def check_dataset(self, dataset):
        """Host-only part of ``check``: the table has one row per box of ``dataset`` and the stamped ``P, H, W`` and
        per-page counts are the dataset's.  ``DeviceDataset.batches(features=)`` calls this."""
        st = self.stamp
        if _dev(dataset.device) != _dev(self.device):
            raise ValueError("feature cache on %s, dataset on %s" % (self.device, dataset.device))
        if (int(dataset.P), int(dataset.H), int(dataset.W)) != (st["P"], st["H"], st["W"]):
            raise ValueError("feature cache built over %d pages of %dx%d, the dataset has %d of %dx%d"
                             % (st["P"], st["H"], st["W"], dataset.P, dataset.H, dataset.W))
        if not np.array_equal(np.asarray(dataset.counts, dtype=np.int64), st["counts"].numpy()):
            raise ValueError("feature cache built over other per-page box counts than the dataset's")
        if len(self) != int(dataset.starts[-1]):
            raise ValueError("feature table of %d rows for a dataset of %d boxes: row ids would not match"
                             % (len(self), int(dataset.starts[-1])))

    def check(self, trainer, dataset):
        """Raise ValueError unless this cache stands for ``trainer``'s conv stack over ``dataset``: the conv stack frozen
        and its BatchNorms in eval mode, the row-shaping configuration, the dataset's shape, counts and box coordinates,
        and every stamped ``convnet.`` tensor bit-equal to the trainer's.  One device comparison and one host read."""
        trainer.check_cached_features()
        st = self.stamp
        if _dev(trainer.device) != _dev(self.device):
            raise ValueError("feature cache on %s, trainer on %s" % (self.device, trainer.device))
        now = stamp_cfg(trainer.cfg)
        if now != st["cfg"]:
            diff = [k for k in now if now[k] != st["cfg"].get(k)]
            raise ValueError("feature cache built with another configuration: %s"
                             % ", ".join("%s=%r (trainer: %r)" % (k, st["cfg"].get(k), now[k]) for k in diff))
        if self.n_vis != engine.backbone_feat(trainer.cfg):
            raise ValueError("feature table of width %d, the configuration has n_vis = %d"
                             % (self.n_vis, engine.backbone_feat(trainer.cfg)))
        self.check_dataset(dataset)
        keys = conv_keys(trainer)
        if keys != list(st["keys"]) or [tuple(_tensor_of(trainer, k).shape) for k in keys] != [tuple(s) for s in st["shapes"]]:
            raise ValueError("feature cache built from a conv stack of another structure")
        a = torch.cat([conv_bits(trainer, keys), _bits(dataset.rows[:, :4])])
        b = torch.cat([st["conv"], _bits(st["boxes"])])
        if a.shape == b.shape and torch.equal(a, b):                          # the one host read
            return
        # the slow path of a refusal: name what differs
        if not torch.equal(_bits(dataset.rows[:, :4]), _bits(st["boxes"])):
            raise ValueError("feature cache built over other box coordinates than the dataset's")
        pos = 0
        for k in keys:
            n = _bits(_tensor_of(trainer, k)).numel()
            if not torch.equal(_bits(_tensor_of(trainer, k)), st["conv"][pos:pos + n]):
                raise ValueError("feature cache is stale: %s differs from the tensor it was built with" % k)
            pos += n
        raise ValueError("feature cache is stale: the conv stack differs from the one it was built with")

    # ------------------------------------------------------------------------------------------------ save / load
    def save(self, path):
        """Table and stamp to ``path`` (torch.save of host tensors and plain values)."""
        st = dict(self.stamp, conv=self.stamp["conv"].cpu(), boxes=self.stamp["boxes"].cpu(),
                  cfg=dict(self.stamp["cfg"], roi_output_size=list(self.stamp["cfg"]["roi_output_size"])),
                  keys=list(self.stamp["keys"]), shapes=[list(s) for s in self.stamp["shapes"]])
        torch.save(dict(format=FORMAT, table=self.table.cpu(), stamp=st), path)

    @classmethod
    def load(cls, path, device):
        """The cache ``save`` wrote, on ``device``.  ``check`` it against the trainer and the dataset before use."""
        blob = torch.load(path, map_location="cpu")
        if not isinstance(blob, dict) or blob.get("format") != FORMAT or "table" not in blob or "stamp" not in blob:
            raise ValueError("%s is not a feature cache of format %d" % (path, FORMAT))
        st = dict(blob["stamp"])
        st["cfg"] = dict(st["cfg"], roi_output_size=tuple(int(x) for x in st["cfg"]["roi_output_size"]))
        st["shapes"] = [tuple(s) for s in st["shapes"]]
        st["conv"], st["boxes"] = st["conv"].to(device), st["boxes"].to(device)
        table = blob["table"].to(device)
        if table.dim() != 2 or table.dtype != torch.float32:
            raise ValueError("%s: the table must be float32 [R, n_vis]" % path)
        return cls(table.contiguous(), st)
