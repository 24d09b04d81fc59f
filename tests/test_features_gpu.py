"""GPU tests of the cached RoI features: cova_feat_rows_gather against numpy indexing (tests/features_oracle.py), a table
above 4 GiB, FeatureCache.build against the direct eval-mode forward, cached train steps / evaluate_split / fit against
the recomputing ones, the launches of a cached step, the refusals and the save / load round trip.

Every comparison is exact: the gather copies bits, and the cached rows come from the very launches the recomputing path
issues (eval-mode kernels whose output elements depend on their own page alone)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, evaluation, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import features_oracle as FO  # noqa: E402
from config_cases import FEATURE_CFG as CFG  # noqa: E402
from helpers import DEV  # noqa: E402

IMG, CS = 96, 3
FROZEN = dict(frozen=("convnet.",), bn_eval=("convnet.",))
SENTINEL = -12345.0


# ---------------------------------------------------------------- 1. the kernel against numpy indexing
@functools.lru_cache(maxsize=None)
def kernel_table(C):
    R = 301
    host = np.random.RandomState(C).standard_normal((R, C)).astype(np.float32)
    return host, torch.from_numpy(host).to(DEV)


def run_gather(table_d, R, C, ids, ld, misalign, rows_behind=2):
    """-> (out [N + rows_behind, ld] as numpy, the sentinel-filled frame around it is checked here)."""
    N = len(ids)
    n_out = (N + rows_behind) * ld
    buf = torch.full((n_out + 12,), SENTINEL, dtype=torch.float32, device=DEV)
    off = 4 + (1 if misalign else 0)                       # torch allocations are 16-byte aligned: 4 floats keep that
    out = buf[off:off + n_out]
    assert (out.data_ptr() % 16 != 0) == bool(misalign)
    ids_d = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(DEV) if N else torch.zeros(1, dtype=torch.int32, device=DEV)
    engine.call("cova_feat_rows_gather", table_d, R, C, ids_d, N, out, ld)
    host = buf.cpu().numpy()
    assert (host[:off] == SENTINEL).all() and (host[off + n_out:] == SENTINEL).all()
    return host[off:off + n_out].reshape(N + rows_behind, ld)


@pytest.mark.parametrize("N", [0, 1, 5, 257, 1441])
@pytest.mark.parametrize("C,ld", [(576, 992), (576, 993), (64, 64), (2304, 2720), (20, 23), (6, 8)])
def test_kernel_equals_numpy_indexing(C, ld, N):
    host, table_d = kernel_table(C)
    R = host.shape[0]
    rs = np.random.RandomState(N + ld)
    ids = rs.randint(0, R, N)                               # repeated ids
    if N >= 5:
        ids[:R] = rs.permutation(R)[:min(N, R)]             # a permuted run
        ids[1], ids[3] = -1, R                              # outside [0, R): rows of zeros
        ids[2] = ids[0]
    elif N == 1:
        ids[0] = R - 1
    ref = FO.gather_rows(host, ids, np.full((N + 2, ld), SENTINEL, np.float32), C)
    if N >= 5:
        assert (ref[1, :C] == 0).all() and (ref[3, :C] == 0).all() and (ref[2, :C] == ref[0, :C]).all()
    got = {m: run_gather(table_d, R, C, ids, ld, m) for m in (False, True)}
    # aligned base: float4 when C % 4 == 0 and ld % 4 == 0; base off by one float: the scalar path -- the same bytes
    for m in (False, True):
        assert np.array_equal(got[m].view(np.int32), ref.view(np.int32)), m
        assert (got[m][:, C:] == SENTINEL).all() and (got[m][N:] == SENTINEL).all()
    assert np.array_equal(got[False].view(np.int32), got[True].view(np.int32))


def test_kernel_refuses_bad_arguments():
    host, table_d = kernel_table(64)
    out = torch.zeros((4, 64), device=DEV)
    ids = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_feat_rows_gather", table_d, 301, 64, ids, 4, out, 63)         # ld_out < C
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_feat_rows_gather", table_d, 301, 0, ids, 4, out, 64)
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_feat_rows_gather", table_d, 301, 64, None, 4, out, 64)
    engine.call("cova_feat_rows_gather", None, 0, 64, None, 0, None, 64)                # N == 0: no launch, no pointers


# ---------------------------------------------------------------- 2. a table above 4 GiB
def test_table_above_4_gib():
    C = 2304
    R = 477700
    assert R * C * 4 >= 4.1 * 2 ** 30
    below = 2 ** 32 // (C * 4) - 1                          # the last row wholly below 4 GiB
    straddle = below + 1
    assert (below + 1) * C * 4 <= 2 ** 32 < (straddle + 1) * C * 4 and straddle * C * 4 < 2 ** 32
    table = torch.empty((R, C), dtype=torch.float32, device=DEV)       # uninitialised: only four rows are written
    want = [0, below, straddle, R - 1]
    vals = torch.from_numpy(np.random.RandomState(1).standard_normal((4, C)).astype(np.float32)).to(DEV)
    for i, r in enumerate(want):
        table[r].copy_(vals[i])
    order = [3, 2, 0, 1, 2]
    ids = torch.tensor([want[i] for i in order], dtype=torch.int32, device=DEV)
    for ld, off in ((C, 0), (C + 1, 0), (C + 4, 1)):                   # the vector path and the scalar path twice
        buf = torch.full((5 * ld + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        out = buf[off:off + 5 * ld]
        engine.call("cova_feat_rows_gather", table, R, C, ids, 5, out, ld)
        got = out.view(5, ld)
        assert torch.equal(got[:, :C], vals[order]), ld
        assert bool((got[:, C:] == SENTINEL).all())
    del table


# ---------------------------------------------------------------- the splits of the cache tests
COUNTS7 = [0, 1, 14, 9, 37, 2, 64]


def make_pages(counts, seed, A=0):
    rs = np.random.RandomState(seed)
    u8 = rs.randint(0, 256, (len(counts), IMG, IMG, 3)).astype(np.uint8)
    rows, addl = [], []
    for n in counts:
        wh = rs.uniform(6, 40, (n, 2))
        xy = rs.uniform(0, 1, (n, 2)) * (IMG - wh)
        lab = np.zeros((n, 1))
        lab[rs.permutation(n)[:3], 0] = [1, 2, 3][:min(n, 3)]
        rows.append(np.concatenate([xy, wh, lab], 1).astype(np.float32))
        addl.append(rs.standard_normal((n, A)).astype(np.float32))
    return u8, rows, (addl if A else None)


def page_set(P=8, seed=4, A=0):
    """tests/trainer_cases.py's page_set with additional features: 11..39 boxes a page, classes 1, 2, 3 once each."""
    counts = [int(c) for c in np.random.RandomState(seed + 100).randint(11, 40, P)]
    return make_pages(counts, seed, A)


def dataset(pages, cs=CS):
    u8, rows, addl = pages
    return DeviceDataset(u8, rows, cs, DEV, additional_feats=addl)


def seeded(cfg=CFG, seed=77):
    skip = ("drop_prob", "roi_op", "sampling_ratio", "roi_aligned", "spatial_scale")
    return weights.seeded_state_dict(seed, logit_gain=2.0, **{k: v for k, v in cfg.items() if k not in skip})


def frozen_trainer(cfg=CFG, **kw):
    return HotPathTrainer(cfg, seeded(cfg), DEV, **dict(FROZEN, **kw))


# ---------------------------------------------------------------- 3. build equals the direct forward
# the configurations of tests/golden/cova_roi2x3_cs1 (non-square bins, n_vis = 384, K = 2) and cova_cs0 (no GAT, T = F = 608)
ROI2X3_CS1 = dict(roi_output_size=(2, 3), hidden_dim=64, bbox_hidden_dim=16)
CS0 = dict(use_context=False, hidden_dim=0, bbox_hidden_dim=32)


@pytest.mark.parametrize("extra,cs", [({}, CS), (dict(roi_op="align"), CS), (dict(backbone_layers=2), CS),
                                      (dict(backbone="resnet50"), CS), (ROI2X3_CS1, 1), (CS0, 0)],
                         ids=["resnet18-pool", "align", "layer2", "resnet50", "roi2x3-cs1", "cs0-no-context"])
def test_build_equals_the_direct_forward(monkeypatch, extra, cs):
    cfg = dict(CFG, **extra)
    tr, ds = frozen_trainer(cfg), dataset(make_pages(COUNTS7, 11), cs)
    n_vis = engine.backbone_feat(cfg)
    batch = next(iter(ds.batches(7, prefetch=False)))
    seen = []
    orig = engine.decoder_fwd
    monkeypatch.setattr(engine, "decoder_fwd", lambda comb, *a, **kw: seen.append(comb) or orig(comb, *a, **kw))
    engine.model_fwd(cfg, tr.params, tr.buffers, batch["images"], batch["bboxes"], batch["additional_feats"],
                     batch["context_indices"], False, save=False)
    monkeypatch.setattr(engine, "decoder_fwd", orig)
    ref = seen[0][:, :n_vis].clone()
    assert ref.shape == (sum(COUNTS7), n_vis) and float(ref.abs().max()) > 0
    for bs in (1, 3, 7):
        cache = FeatureCache.build(tr, ds, batch_size=bs, prefetch=bs != 3)
        assert cache.table.shape == ref.shape and cache.nbytes == ref.numel() * 4
        assert torch.equal(cache.table, ref), bs
        cache.check(tr, ds)
    # the forward from the cached visual features is the full forward, bit for bit
    order = np.asarray([6, 2, 4, 1])
    full = next(iter(ds.batches(4, order=order, prefetch=False)))
    cached = next(iter(ds.batches(4, order=order, features=cache)))
    assert "images" not in cached and tuple(full["context_indices"].shape) == ((COUNTS7[6] + COUNTS7[2] + COUNTS7[4] + 1,
                                                                               2 * cs) if cfg["use_context"] else (0, 0))
    assert torch.equal(tr.predict(cached)[0], tr.predict(full)[0])
    assert torch.equal(tr.loss(cached), tr.loss(full))


# ---------------------------------------------------------------- 4. cached steps equal recomputed steps
def run_steps(cfg, pages, cached, shard):
    tr, ds = frozen_trainer(cfg), dataset(pages)
    cache = FeatureCache.build(tr, ds) if cached else None
    if cached:
        cache.check(tr, ds)
    losses, preds, n_batches = [], [], 0
    epoch = 0
    while n_batches < 4:
        epoch += 1
        for b in ds.batches(3, shuffle=True, sampling_fraction=0.9, seed=21, epoch=epoch, features=cache, **shard):
            assert ("images" in b) != cached and ("visual_feats" in b) == cached
            if cached:
                table, ids = b["visual_feats"]
                assert table is cache.table and ids.dtype == torch.int32 and ids.shape[0] == b["bboxes"].shape[0]
            loss, pred = tr.train_step(b)
            losses.append(loss.clone())
            preds.append(pred.clone())
            n_batches += 1
            if n_batches == 4:
                break
    return tr, torch.cat(losses), torch.cat(preds)


@pytest.mark.parametrize("A,shard", [(0, {}), (1, {}), (0, dict(rank=1, world_size=2))],
                         ids=["T-aligned", "T-odd-scalar-path", "rank1-of-2"])
def test_cached_steps_equal_recomputed_steps(A, shard):
    cfg = dict(CFG, n_additional_feat=A)
    T = 576 + 16 + A + 48
    assert (T % 4 == 0) == (A == 0)
    pages = page_set(P=8, seed=4, A=A)
    a, la, pa = run_steps(cfg, pages, False, shard)
    b, lb, pb = run_steps(cfg, pages, True, shard)
    assert a.step_count == b.step_count == 4
    assert torch.equal(la, lb) and torch.equal(pa, pb) and bool(torch.isfinite(la).all())
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
    for k in a.buffers:
        assert torch.equal(a.buffers[k], b.buffers[k]), k
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    sd = seeded(cfg)
    assert not torch.equal(a.params["decoder.5.weight"], sd["decoder.5.weight"].to(DEV))        # the head did train
    assert torch.equal(a.params["convnet.0.weight"], sd["convnet.0.weight"].to(DEV))


def test_unsampled_batches_carry_the_dataset_rows():
    pages = make_pages(COUNTS7, 11)
    tr, ds = frozen_trainer(), dataset(pages)
    cache = FeatureCache.build(tr, ds, batch_size=7)
    plan = [[5, 0, 6], [2, 1, 4], [3]]
    order = np.concatenate(plan)
    for ids, b in zip(plan, ds.batches(3, order=order, features=cache)):
        ref = FO.kept_row_ids(ds.starts, ids, [np.arange(COUNTS7[p]) for p in ids])
        assert np.array_equal(b["visual_feats"][1].cpu().numpy(), ref)
        logits, _ = tr.predict(b)
        full = next(iter(ds.batches(len(ids), order=np.asarray(ids), prefetch=False)))
        assert torch.equal(logits, tr.predict(full)[0])
        assert torch.equal(tr.loss(b), tr.loss(full))


# ---------------------------------------------------------------- 5. launches
def test_a_cached_step_launches_one_gather_and_no_conv_stack():
    tr, ds = frozen_trainer(), dataset(page_set(P=3))
    cache = FeatureCache.build(tr, ds)
    batches = {c: next(iter(ds.batches(3, prefetch=False, features=cache if c else None))) for c in (False, True)}
    counts = {}
    for c in (False, True):
        _lib.PROFILE = {name: [] for name in _lib.lib().fn}
        try:
            tr.train_step(batches[c])
            torch.cuda.synchronize()
            counts[c] = {k: len(v) for k, v in _lib.PROFILE.items() if v}
        finally:
            _lib.PROFILE = None
    heavy = ("cova_conv", "cova_roipool", "cova_roialign", "cova_bn_relu_maxpool", "cova_pages_u8_gather_f32")
    assert any(k.startswith("cova_conv") for k in counts[False]) and any(k.startswith("cova_roipool") for k in counts[False])
    assert [k for k in counts[True] if k.startswith(heavy)] == []
    assert counts[True]["cova_feat_rows_gather"] == 1 and "cova_feat_rows_gather" not in counts[False]
    # everything else of the step is what the recomputing step launches
    rest = {k: v for k, v in counts[False].items() if not k.startswith(heavy) and k != "cova_bn_eval_params"}
    assert {k: v for k, v in counts[True].items() if k != "cova_feat_rows_gather"} == rest
    # ... and assembling a cached batch gathers no page
    _lib.PROFILE = {name: [] for name in _lib.lib().fn}
    try:
        for _ in ds.batches(2, prefetch=False, features=cache):
            pass
        assert not _lib.PROFILE["cova_pages_u8_gather_f32"] and len(_lib.PROFILE["cova_sample_boxes"]) == 2
    finally:
        _lib.PROFILE = None


# ---------------------------------------------------------------- 6. evaluate_split
def refuse_host_reads(monkeypatch, allowed):
    """Tensor.cpu / item / numpy / tolist raise unless ``allowed[0]`` > 0."""
    orig = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "numpy", "tolist")}

    def guard(name):
        def f(self, *a, **kw):
            if allowed[0] <= 0 and (name != "numpy" or self.is_cuda):
                raise AssertionError("host read (%s) where none is allowed" % name)
            return orig[name](self, *a, **kw)
        return f
    for n in orig:
        monkeypatch.setattr(torch.Tensor, n, guard(n))


def allowing(fn, allowed, calls):
    def f(*a, **kw):
        allowed[0] += 1
        calls.append(1)
        try:
            return fn(*a, **kw)
        finally:
            allowed[0] -= 1
    return f


@pytest.mark.parametrize("with_loss", [False, True])
def test_evaluate_split_with_the_cache_equals_the_uncached_call(monkeypatch, with_loss):
    tr, ds = frozen_trainer(label_smoothing=0.1), dataset(page_set(P=23, seed=6))
    cache = FeatureCache.build(tr, ds)
    ref = evaluate_split(tr, ds, with_loss=with_loss)
    allowed, copies, checks = [0], [], []
    refuse_host_reads(monkeypatch, allowed)
    monkeypatch.setattr(evaluation, "_read_tables", allowing(evaluation._read_tables, allowed, copies))
    monkeypatch.setattr(FeatureCache, "check", allowing(FeatureCache.check, allowed, checks))      # on entry, once
    with pytest.raises(AssertionError, match="host read"):
        torch.zeros(1, device=DEV).item()
    for kw in (dict(), dict(prefetch=False, batch_size=7)):
        del copies[:], checks[:]
        rep = evaluate_split(tr, ds, with_loss=with_loss, features=cache, **kw)
        assert len(copies) == 1 and len(checks) == 1
        assert rep.evaluated.all()
        if not kw:
            assert np.array_equal(rep.ranks, ref.ranks) and np.array_equal(rep.top1, ref.top1)
            assert rep.loss == ref.loss
            if with_loss:
                assert np.array_equal(rep.confusion, ref.confusion)
                for k in ("kept", "bad_labels", "loss_numerator", "loss_denominator"):
                    assert rep.metrics[k] == ref.metrics[k], k
    parts = [evaluate_split(tr, ds, rank=r, world_size=2, merge=False, features=cache) for r in (0, 1)]
    merged = evaluation.EvalReport.merge(parts)
    whole = [evaluate_split(tr, ds, rank=r, world_size=2, merge=False) for r in (0, 1)]
    assert np.array_equal(merged.ranks, evaluation.EvalReport.merge(whole).ranks)


# ---------------------------------------------------------------- 7. fit
def test_fit_with_caches_equals_fit_without():
    train, val = dataset(page_set(P=9, seed=4)), dataset(page_set(P=17, seed=9))
    a, b = (frozen_trainer(lr=2e-3, track_metrics=True) for _ in range(2))
    kw = dict(sampling_fraction=0.9, seed=12, eval_interval=2, k=3, lr_schedule=evaluation.step_lr(2, 0.5))
    ref = fit(a, train, val, 3, 3, **kw)
    tc, vc = FeatureCache.build(b, train), FeatureCache.build(b, val, batch_size=4)
    got = fit(b, train, val, 3, 3, train_features=tc, val_features=vc, **kw)
    assert got[:4] == ref[:4] and len(got.history) == len(ref.history) == 3
    for g, r in zip(got.history, ref.history):
        assert set(g) == set(r)
        for key in r:
            if key == "seconds":
                continue
            if key == "class_acc":
                assert (g[key] is None) == (r[key] is None) and (r[key] is None or np.array_equal(g[key], r[key]))
            else:
                assert g[key] == r[key], (r["epoch"], key)
    assert ref.history[0]["boxes"] > 0 and ref.history[0]["eval_acc"] is not None
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.exp_avg, b.exp_avg) and a.step_count == b.step_count


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    pages = page_set(P=4)
    ds, tr = dataset(pages), frozen_trainer()
    cache = FeatureCache.build(tr, ds)
    batch = next(iter(ds.batches(4, prefetch=False, features=cache)))
    sd = seeded()
    # a trainable conv stack; a convnet. BatchNorm in train mode
    for kw, msg in ((dict(bn_eval=("convnet.",)), "frozen conv stack"), (dict(frozen=("convnet.",)), "eval mode")):
        other = HotPathTrainer(CFG, sd, DEV, **kw)
        before = other.step_count
        with pytest.raises(ValueError, match=msg):
            other.train_step(batch)
        assert other.step_count == before
        with pytest.raises(ValueError, match=msg):
            cache.check(other, ds)
        with pytest.raises(ValueError, match=msg):
            FeatureCache.build(other, ds)
        with pytest.raises(ValueError, match=msg):
            evaluate_split(other, ds, features=cache)
    # one conv weight / one running_mean changed
    for key in ("convnet.4.0.conv1.weight", "convnet.4.1.bn2.running_mean"):
        other = frozen_trainer()
        cache.check(other, ds)
        t = other.params[key] if key in other.params else other.buffers[key]
        t.view(-1)[5] += 1e-3
        with pytest.raises(ValueError, match="stale: " + key.replace(".", r"\.")):
            cache.check(other, ds)
        with pytest.raises(ValueError, match="stale"):
            fit(HotPathTrainer(CFG, other.state_dict(), DEV, track_metrics=True, **FROZEN), ds, ds, 1, 2,
                train_features=cache)
    # a dataset with other counts, on the host
    u8, rows, _ = pages
    fewer = DeviceDataset(u8, [rows[0][:-1]] + rows[1:], CS, DEV)
    with pytest.raises(ValueError, match="box counts"):
        cache.check(tr, fewer)
    with pytest.raises(ValueError, match="box counts"):
        fewer.batches(2, features=cache)
    with pytest.raises(ValueError, match="box counts"):
        evaluate_split(tr, fewer, features=cache)
    # save=True with a plan that holds "convstack"
    args = (CFG, tr.params, tr.buffers, None, batch["bboxes"], batch["additional_feats"], batch["context_indices"])
    for plan in (None, engine.full_plan(tr.params)):
        with pytest.raises(ValueError, match="convstack"):
            engine.model_fwd(*args, tr.modes, save=True, plan=plan, visual_feats=batch["visual_feats"])
    logits, sv = engine.model_fwd(*args, tr.modes, save=True, plan=tr.plan, visual_feats=batch["visual_feats"])
    assert sv["conv"] is None and sv["roi"] is None and logits.shape == (batch["bboxes"].shape[0], 4)
    # a row_ids / table mismatch, caught on the host
    table, ids = batch["visual_feats"]
    for vis, msg in (((table, ids[:-1]), "row ids for"), ((table[:, :512].contiguous(), ids), "dense float32"),
                     ((table, ids.long()), "int32")):
        with pytest.raises(ValueError, match=msg):
            tr.predict(dict(batch, visual_feats=vis))
    with pytest.raises(RuntimeError, match="without images"):
        tr.predict({k: v for k, v in batch.items() if k != "visual_feats"})


# ---------------------------------------------------------------- 9. save / load
def test_save_load_round_trip(tmp_path):
    tr, ds = frozen_trainer(), dataset(make_pages(COUNTS7, 11))
    cache = FeatureCache.build(tr, ds)
    path = str(tmp_path / "features.pt")
    cache.save(path)
    back = FeatureCache.load(path, DEV)
    assert back.table.is_cuda and torch.equal(back.table, cache.table) and back.nbytes == cache.nbytes == 127 * 576 * 4
    assert set(back.stamp) == set(cache.stamp)
    for k, v in cache.stamp.items():
        if torch.is_tensor(v):
            assert v.dtype == back.stamp[k].dtype and v.device == back.stamp[k].device and torch.equal(v, back.stamp[k]), k
        else:
            assert v == back.stamp[k], k
    back.check(tr, ds)
    ref = evaluate_split(tr, ds, batch_size=3)
    rep = evaluate_split(tr, ds, batch_size=3, features=back)
    assert np.array_equal(rep.ranks, ref.ranks) and np.array_equal(rep.top1, ref.top1)
