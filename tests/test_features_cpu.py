"""Host-only validation of the cached-feature path: the shape contract of ``visual_feats``, the trainer's host flags, the
stamp of a FeatureCache (configuration, dataset, conv-stack tensors) and its save / load round trip -- all on CPU tensors --
plus the numpy oracle's own semantics and the header's declaration of the entry point."""
import ctypes
import types

import numpy as np
import pytest
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, engine, features, weights
from cova_web_object_detection_amd.features import FeatureCache
from cova_web_object_detection_amd.trainer import HotPathTrainer
import features_oracle as FO
from config_cases import FEATURE_CFG as CFG

FROZEN = dict(frozen=("convnet.",), bn_eval=("convnet.",))


def trainer(cfg=CFG, seed=3, **kw):
    sd = weights.seeded_state_dict(seed, **{k: v for k, v in cfg.items() if k not in ("drop_prob", "roi_op")})
    return HotPathTrainer(cfg, sd, "cpu", **kw)


def fake_dataset(counts=(0, 1, 14, 9), H=96, W=96, seed=0):
    counts = np.asarray(counts, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = torch.from_numpy(np.random.RandomState(seed).uniform(0, 50, (int(starts[-1]), 5)).astype(np.float32))
    return types.SimpleNamespace(P=len(counts), H=H, W=W, counts=counts, starts=starts, rows=rows,
                                 device=torch.device("cpu"))


def cache_for(tr, ds):
    table = torch.zeros((int(ds.starts[-1]), engine.backbone_feat(tr.cfg)))
    return FeatureCache(table, FeatureCache.make_stamp(tr, ds))


def test_header_declares_the_entry_point():
    protos = _lib.parse_header()
    p, i = ctypes.c_void_p, ctypes.c_int
    assert protos["cova_feat_rows_gather"] == [p, ctypes.c_longlong, i, p, i, p, i, p]


def test_oracle_semantics():
    table = np.arange(12, dtype=np.float32).reshape(4, 3)
    out = np.full((4, 5), -7.0, dtype=np.float32)
    got = FO.gather_rows(table, [2, -1, 4], out, C=2)
    assert got.tolist() == [[6, 7, -7, -7, -7], [0, 0, -7, -7, -7], [0, 0, -7, -7, -7], [-7] * 5]
    assert (out == -7).all()
    assert FO.kept_row_ids([0, 0, 1, 15], [2, 0, 1], [[0, 3], [], [0]]).tolist() == [1, 4, 0]


def test_visual_feats_contract():
    n_vis = engine.backbone_feat(CFG)
    assert n_vis == 576
    table, ids = torch.zeros((9, n_vis)), torch.zeros(5, dtype=torch.int32)
    assert engine.check_visual_feats(CFG, (table, ids), 5)[0] is table
    bad = [((table, ids), 4, "5 row ids for 4 boxes"),
           ((table[:, :575], ids), 5, "dense float32"),
           ((table.double(), ids), 5, "dense float32"),
           ((table, ids.long()), 5, "int32"),
           ((table, ids.view(5, 1)), 5, "int32"),
           ((table[:0], ids), 5, "empty table"),
           (table, 5, "must be"),
           ((table, ids, ids), 5, "must be")]
    for vis, n, msg in bad:
        with pytest.raises(ValueError, match=msg):
            engine.check_visual_feats(CFG, vis, n)
    # check_batch takes the image-less form only with the features
    bb, af, ctx = torch.zeros((5, 5)), torch.zeros((5, 0)), torch.zeros((5, 6), dtype=torch.int64)
    engine.check_batch(CFG, None, bb, af, ctx, False, (table, ids))
    with pytest.raises(RuntimeError, match="without images"):
        engine.check_batch(CFG, None, bb, af, ctx, False)
    with pytest.raises(ValueError, match="row ids"):
        engine.check_batch(CFG, None, bb, af, ctx, False, (table, ids[:4]))
    engine.check_batch(CFG, torch.zeros((1, 3, 8, 8)), bb, af, ctx, False)            # today's form is unchanged


def test_trainer_flags():
    ok = trainer(**FROZEN)
    assert ok.conv_frozen and ok.conv_bn_eval
    ok.check_cached_features()
    with pytest.raises(ValueError, match="frozen conv stack"):
        trainer(bn_eval=("convnet.",)).check_cached_features()
    with pytest.raises(ValueError, match="frozen conv stack"):
        trainer(frozen=("convnet.4.",), bn_eval=("convnet.",)).check_cached_features()
    with pytest.raises(ValueError, match="eval mode"):
        trainer(frozen=("convnet.",)).check_cached_features()
    with pytest.raises(ValueError, match="eval mode"):
        trainer(frozen=("convnet.",), bn_eval=("convnet.4.",)).check_cached_features()      # the stem's stays in train mode


def test_stamp_cfg_defaults_and_fields():
    assert features.stamp_cfg(CFG) == dict(backbone="resnet18", backbone_layers=1, roi_output_size=(3, 3), roi_op="pool",
                                           sampling_ratio=2, roi_aligned=False, spatial_scale=None)
    assert features.stamp_cfg(dict(CFG, roi_output_size=[3, 3], spatial_scale=0)) == features.stamp_cfg(CFG)
    for k, v in dict(backbone="resnet50", backbone_layers=2, roi_output_size=(2, 3), roi_op="align", sampling_ratio=3,
                     roi_aligned=True, spatial_scale=0.25).items():
        assert features.stamp_cfg(dict(CFG, **{k: v})) != features.stamp_cfg(CFG), k
    assert features.stamp_cfg(dict(CFG, hidden_dim=96, drop_prob=0.0)) == features.stamp_cfg(CFG)   # the head is free


def test_check_accepts_its_own_trainer_and_refuses_every_difference():
    tr, ds = trainer(**FROZEN), fake_dataset()
    cache = cache_for(tr, ds)
    assert cache.nbytes == 24 * 576 * 4 and len(cache) == 24 and cache.n_vis == 576
    cache.check(tr, ds)
    cache.check(trainer(dict(CFG, hidden_dim=32), **FROZEN), ds)                    # another head, the same conv stack
    with pytest.raises(ValueError, match="frozen conv stack"):
        cache.check(trainer(bn_eval=("convnet.",)), ds)
    with pytest.raises(ValueError, match="eval mode"):
        cache.check(trainer(frozen=("convnet.",)), ds)
    with pytest.raises(ValueError, match="another configuration: roi_op"):
        cache.check(trainer(dict(CFG, roi_op="align"), **FROZEN), ds)
    # one conv weight, one running_mean, one num_batches_tracked
    for key in ("convnet.4.1.conv2.weight", "convnet.1.running_mean", "convnet.4.0.bn1.num_batches_tracked"):
        other = trainer(**FROZEN)
        t = other.params[key] if key in other.params else other.buffers[key]
        t.view(-1)[-1] += 1
        with pytest.raises(ValueError, match="stale: " + key.replace(".", r"\.")):
            cache.check(other, ds)
    with pytest.raises(ValueError, match="stale"):
        cache.check(trainer(seed=4, **FROZEN), ds)
    # the dataset
    with pytest.raises(ValueError, match="box counts"):
        cache.check(tr, fake_dataset((0, 1, 9, 14)))
    with pytest.raises(ValueError, match="pages of"):
        cache.check(tr, fake_dataset((0, 1, 14, 9, 0)))
    with pytest.raises(ValueError, match="pages of"):
        cache.check(tr, fake_dataset(H=128))
    with pytest.raises(ValueError, match="box coordinates"):
        cache.check(tr, fake_dataset(seed=1))
    moved = fake_dataset()
    moved.rows[3, 4] = 2.0                                                          # a label is not a coordinate
    cache.check(tr, moved)
    with pytest.raises(ValueError, match="row ids would not match"):
        FeatureCache(cache.table[:-1], cache.stamp).check_dataset(ds)


def test_save_load_round_trip_on_the_host(tmp_path):
    tr, ds = trainer(**FROZEN), fake_dataset()
    cache = cache_for(tr, ds)
    cache.table.copy_(torch.from_numpy(np.random.RandomState(2).standard_normal(tuple(cache.table.shape)).astype(np.float32)))
    path = str(tmp_path / "cache.pt")
    cache.save(path)
    back = FeatureCache.load(path, "cpu")
    assert torch.equal(back.table, cache.table) and back.nbytes == cache.nbytes
    assert set(back.stamp) == set(cache.stamp)
    for k, v in cache.stamp.items():
        if torch.is_tensor(v):
            assert v.dtype == back.stamp[k].dtype and torch.equal(v, back.stamp[k]), k
        else:
            assert v == back.stamp[k], k
    back.check(tr, ds)
    torch.save(dict(format=0), path)
    with pytest.raises(ValueError, match="not a feature cache"):
        FeatureCache.load(path, "cpu")
