"""GPU tests of the spatial context graphs: cova_context_knn through the C ABI against the numpy oracle
(tests/graph_oracle.py), the hybrid table against cova_collate_boxes' window, DeviceCollate / DeviceDataset(spatial_k=)
against the oracle run over the kept boxes, the untouched default, and the graph through the model (train steps, the GAT
layer on a hub of in-degree 130, evaluate_split, fit, the feature cache shared by two graphs).

The graph is integer output decided by integer compares of float32 bit patterns: every comparison of tables is
np.array_equal on int64."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, pipeline  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import GraphAttentionLayer  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceCollate, DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
import graph_oracle as GO  # noqa: E402
import sampling_oracle as SO  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from helpers import DEV, profiled, random_xyxy as random_boxes, relerr  # noqa: E402
from trainer_cases import page_set, seeded  # noqa: E402

GUARD = -7


# ---------------------------------------------------------------- 1. the kernel against the oracle, through the C ABI
def as_batch(pages):
    """list of [n,4] pages -> (bboxes [N,5] = page,x1,y1,x2,y2, page_start [B+1])."""
    ps = np.concatenate([[0], np.cumsum([p.shape[0] for p in pages])]).astype(np.int64)
    bb = [np.concatenate([np.full((p.shape[0], 1), i, np.float32), p.reshape(-1, 4)], 1) for i, p in enumerate(pages)]
    return np.concatenate(bb, 0).astype(np.float32), ps


def run_knn(bboxes, page_start, cs, k):
    """cova_context_knn into a table framed by guard rows; every slot of the table must have been written."""
    N, B, K = bboxes.shape[0], len(page_start) - 1, 2 * cs + k
    bb = torch.from_numpy(np.ascontiguousarray(bboxes)).to(DEV)
    offs = torch.from_numpy(np.asarray(page_start, dtype=np.int32)).to(DEV)
    buf = torch.full((N + 4, K), GUARD, dtype=torch.int64, device=DEV)
    engine.call("cova_context_knn", bb, offs, B, N, cs, k, buf[2:])
    host = buf.cpu().numpy()
    assert (host[:2] == GUARD).all() and (host[N + 2:] == GUARD).all()
    got = host[2:N + 2]
    assert (got != GUARD).all()
    return got


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """-> (bboxes, page_start, cs, k, oracle table); computed once per case."""
    rs = np.random.RandomState(len(name) * 7 + 3)
    if name == "mixed_pages":                      # n-1 < k, n-1 == k (n = 25), n-1 > k; an empty page in the middle
        pages, cs, k = [random_boxes(rs, n) for n in (0, 1, 2, 25, 0, 65, 130)], 0, 24
    elif name == "tie_grid":
        pages, cs, k = [GO.tie_grid()], 0, 8
    elif name == "identical_boxes":                # every key ties: the order is the index alone
        pages, cs, k = [np.tile(np.asarray([[10, 20, 50, 40]], np.float32), (70, 1)), random_boxes(rs, 9)], 0, 24
    elif name == "zero_area_boxes":                # points and segments on a coarse integer lattice
        p = rs.randint(0, 12, (90, 2)).astype(np.float32) * 8
        q = p.copy()
        q[::3, 0] += 16                            # every third one a horizontal segment
        pages, cs, k = [np.concatenate([p, q], 1)], 0, 24
    elif name == "n300_k48":
        pages, cs, k = [random_boxes(rs, 300, 1280.0), random_boxes(rs, 257, 1280.0)], 0, 48
    elif name == "n5000_k4":                       # far beyond the keys a lane holds in registers
        pages, cs, k = [random_boxes(rs, 5000, 1280.0)], 0, 4
    elif name == "hybrid_wide":                    # window + neighbours, a page of 256 and one of 257 boxes
        pages, cs, k = [random_boxes(rs, 256), random_boxes(rs, 257), random_boxes(rs, 14)], 6, 12
    else:
        raise KeyError(name)
    bb, ps = as_batch(pages)
    return bb, ps, cs, k, GO.batch_graph(bb, ps, cs, k)


@pytest.mark.parametrize("name", ["mixed_pages", "tie_grid", "identical_boxes", "zero_area_boxes", "n300_k48", "n5000_k4",
                                  "hybrid_wide"])
def test_kernel_equals_the_oracle(name):
    bb, ps, cs, k, ref = kernel_case(name)
    got = run_knn(bb, ps, cs, k)
    assert got.dtype == np.int64 and got.shape == ref.shape
    assert np.array_equal(got, ref)
    if name == "mixed_pages":
        assert (ref[0] == -1).all()                                             # the one-box page: pads alone
        n25 = ref[int(ps[3]):int(ps[4])]
        assert (n25 >= 0).all() and (ref[int(ps[5])] >= 0).all() and (ref[1, 1:] == -1).all()
    if name == "identical_boxes":
        assert ref[0].tolist() == list(range(1, 25)) and ref[5, :6].tolist() == [0, 1, 2, 3, 4, 6]
    if name == "tie_grid":
        assert np.bincount(ref[ref >= 0], minlength=131)[130] == 130            # the hub of the GAT test below
    assert np.array_equal(run_knn(bb, ps, cs, k), got)                          # a second launch: the same bits


def test_kernel_is_safe_and_valid_on_non_finite_boxes():
    rs = np.random.RandomState(2)
    pages = [random_boxes(rs, 40), random_boxes(rs, 70)]
    pages[0][3] = np.nan
    pages[0][7, 2] = np.inf
    pages[1][::5, 0] = -np.inf
    pages[1][1] = [np.nan, 0, np.inf, -np.inf]
    bb, ps = as_batch(pages)
    got = run_knn(bb, ps, 2, 30)
    for p in range(2):
        lo, hi = int(ps[p]), int(ps[p + 1])
        for i, row in enumerate(got[lo:hi]):
            ids = row[row >= 0]
            assert (row >= -1).all() and ((ids >= lo) & (ids < hi)).all()
            assert len(set(ids.tolist())) == ids.shape[0] and lo + i not in ids
            win = min(i, 2) + min(hi - lo - 1 - i, 2)
            assert ids.shape[0] == win + min(30, hi - lo - 1 - win)             # every slot a candidate can fill is filled


def test_entry_point_refuses_bad_arguments_and_skips_empty_work():
    bb = torch.zeros((4, 5), device=DEV)
    offs = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    ctx = torch.full((4, 6), GUARD, dtype=torch.int64, device=DEV)
    for cs, k in ((-1, 4), (1, -1), (512, 1)):
        with pytest.raises(_lib.CovaHipError):
            engine.call("cova_context_knn", bb, offs, 1, 4, cs, k, ctx)
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_context_knn", bb, None, 1, 4, 1, 4, ctx)
    engine.call("cova_context_knn", None, None, 1, 0, 1, 4, None)               # N == 0: no launch, no pointers
    engine.call("cova_context_knn", None, None, 1, 4, 0, 0, None)               # a table of width 0 likewise
    torch.cuda.synchronize()
    assert (ctx == GUARD).all()


# ---------------------------------------------------------------- 2. hybrid rows against cova_collate_boxes' window
def make_rows(rs, n, size=200.0):
    r = np.zeros((n, 5), np.float32)
    r[:, :2] = rs.uniform(0, size, (n, 2))
    r[:, 2:4] = rs.uniform(2, 60, (n, 2))
    r[rs.permutation(n)[:min(3, n)], 4] = [1, 2, 3][:min(3, n)]
    return r


def test_hybrid_table_extends_the_collate_window_without_repeats():
    rs = np.random.RandomState(12)
    counts = [30, 3, 0, 14, 77, 1]
    u8 = rs.randint(0, 256, (len(counts), 8, 8, 3)).astype(np.uint8)
    rows = [make_rows(rs, n) for n in counts]
    cs, k = 6, 12
    window = DeviceCollate(cs, DEV)(u8, rows)
    got, launches = profiled(lambda: DeviceCollate(cs, DEV, spatial_k=k)(u8, rows))
    assert launches == {"cova_images_u8_to_f32": 1, "cova_collate_boxes": 1, "cova_context_knn": 1}
    for key in ("images", "bboxes", "labels", "additional_feats", "page_start"):
        assert torch.equal(got[key], window[key]), key
    ctx, win = got["context_indices"].cpu().numpy(), window["context_indices"].cpu().numpy()
    assert ctx.dtype == np.int64 and ctx.shape == (sum(counts), 2 * cs + k) and win.shape == (sum(counts), 2 * cs)
    assert np.array_equal(ctx[:, :2 * cs], win)                                  # columns 0..12 are the collate table
    ps = got["page_start"].cpu().numpy()
    assert np.array_equal(ctx, GO.batch_graph(got["bboxes"].cpu().numpy(), ps, cs, k))
    for p in range(len(counts)):
        for g in range(int(ps[p]), int(ps[p + 1])):
            ids = ctx[g][ctx[g] >= 0]
            assert len(set(ids.tolist())) == ids.shape[0]                        # no repeated neighbour
            members = set(win[g][win[g] >= 0].tolist()) | {g}
            assert not members & set(ctx[g, 2 * cs:].tolist())                   # no spatial column holds i or a window member
            assert ids.shape[0] == min(counts[p] - 1, (win[g] >= 0).sum() + k)
    # cs = 12, k = 0 through the new entry point is the collate table outright
    w12 = DeviceCollate(12, DEV)(u8, rows)
    assert np.array_equal(run_knn(w12["bboxes"].cpu().numpy(), ps, 12, 0), w12["context_indices"].cpu().numpy())
    # sampled collation: the graph runs over the kept boxes
    smp = DeviceCollate(cs, DEV, spatial_k=k, sampling_fraction=0.5, seed=3)(u8, rows, page_ids=[9, 8, 7, 6, 5, 4], epoch=2)
    ref = DeviceCollate(cs, DEV, sampling_fraction=0.5, seed=3)(u8, rows, page_ids=[9, 8, 7, 6, 5, 4], epoch=2)
    assert torch.equal(smp["bboxes"], ref["bboxes"]) and smp["bboxes"].shape[0] < sum(counts)
    sctx = smp["context_indices"].cpu().numpy()
    assert np.array_equal(sctx[:, :2 * cs], ref["context_indices"].cpu().numpy())
    assert np.array_equal(sctx, GO.batch_graph(smp["bboxes"].cpu().numpy(), smp["page_start"].cpu().numpy(), cs, k))


# ---------------------------------------------------------------- 3. the dataset path
def small_dataset(P=13, H=16, W=20, seed=21):
    rs = np.random.RandomState(seed)
    u8 = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    counts = rs.randint(0, 60, P).tolist()
    counts[1], counts[4] = 1, 0
    return u8, [make_rows(rs, n) for n in counts]


def kept_boxes(rows, sf, seed, epoch, pid):
    """x1,y1,x2,y2 of the boxes page ``pid`` keeps (sampling_oracle.select over the hash keys), float32 adds."""
    r = rows[pid]
    idx = np.arange(r.shape[0]) if sf == 1.0 else SO.select(r, int(sf * r.shape[0]), SO.hash_keys(seed, epoch, pid, r.shape[0]))
    r = r[idx]
    return np.concatenate([r[:, 0:2], r[:, 0:2] + r[:, 2:4]], 1).astype(np.float32)


@pytest.mark.parametrize("sf", [1.0, 0.9, 0.5])
@pytest.mark.parametrize("cs,k", [(0, 24), (4, 9)])
def test_dataset_batches_equal_the_oracle_over_the_kept_boxes(sf, cs, k):
    u8, rows = small_dataset()
    ds = DeviceDataset(u8, rows, cs, DEV, spatial_k=k)
    seed, epoch, n = 17, 2, 0
    for got in ds.batches(5, shuffle=True, sampling_fraction=sf, seed=seed, epoch=epoch):
        ids = got["page_ids"].cpu().tolist()
        pages = [kept_boxes(rows, sf, seed, epoch, p) for p in ids]
        bb, ps = as_batch(pages)
        assert np.array_equal(got["bboxes"].cpu().numpy(), bb) and np.array_equal(got["page_start"].cpu().numpy(), ps)
        ctx = got["context_indices"].cpu().numpy()
        assert ctx.dtype == np.int64 and ctx.shape == (bb.shape[0], 2 * cs + k)
        assert np.array_equal(ctx, GO.batch_graph(bb, ps, cs, k))
        n += 1
    assert n == 3
    if sf < 1.0:
        assert sum(b["labels"].numel() for b in ds.batches(13, sampling_fraction=sf, seed=seed, epoch=epoch)) \
            < sum(r.shape[0] for r in rows)                                      # something was dropped


def epoch_tensors(ds, **kw):
    out = []
    for b in ds.batches(**kw):
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    torch.cuda.synchronize()
    return out


def test_dataset_graphs_are_reproducible_and_prefetch_changes_nothing():
    u8, rows = small_dataset()
    ds = DeviceDataset(u8, rows, 3, DEV, spatial_k=10)
    kw = dict(batch_size=3, shuffle=True, sampling_fraction=0.9, seed=5, epoch=1)
    a, b, c = epoch_tensors(ds, prefetch=True, **kw), epoch_tensors(ds, prefetch=False, **kw), epoch_tensors(ds, prefetch=True, **kw)
    assert len(a) == len(b) == len(c) == 5
    for x, y, z in zip(a, b, c):
        for key in ("images", "bboxes", "labels", "context_indices", "additional_feats", "page_start", "page_ids"):
            assert torch.equal(x[key], y[key]) and torch.equal(x[key], z[key]), key
        assert x["context_indices"].shape[1] == 16


def test_a_pages_graph_does_not_depend_on_batch_size_position_or_rank():
    u8, rows = small_dataset()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=7)

    def local(**kw):
        out = {}
        for x in ds.batches(sampling_fraction=0.5, seed=3, epoch=7, **kw):
            ps, ctx = x["page_start"].tolist(), x["context_indices"].cpu().numpy()
            for i, p in enumerate(x["page_ids"].tolist()):
                t = ctx[ps[i]:ps[i + 1]]
                out[p] = np.where(t >= 0, t - ps[i], -1)
        return out
    ref = local(batch_size=13)
    assert set(ref) == set(range(13))
    for p, t in ref.items():
        assert np.array_equal(t, GO.page_graph(kept_boxes(rows, 0.5, 3, 7, p), 2, 7))
    for kw in (dict(batch_size=1), dict(batch_size=5), dict(batch_size=4, order=list(range(12, -1, -1))),
               dict(batch_size=3, shuffle=True), dict(batch_size=2, rank=1, world_size=2, order=list(range(13)) + [0])):
        got = local(**kw)
        assert got and set(got) <= set(ref)
        for p, t in got.items():
            assert np.array_equal(t, ref[p]), (kw, p)


def test_with_context_shares_the_resident_split():
    u8, rows = small_dataset()
    ds = DeviceDataset(u8, rows, 12, DEV)
    before = torch.cuda.memory_allocated()
    sib = ds.with_context(0, 24)
    assert torch.cuda.memory_allocated() == before
    assert sib.store.data_ptr() == ds.store.data_ptr() and sib.rows.data_ptr() == ds.rows.data_ptr()
    assert sib.img_ids is ds.img_ids and (sib.cs, sib.ks, ds.cs, ds.ks) == (0, 24, 12, 0)
    a = next(iter(sib.batches(13, prefetch=False)))
    b = next(iter(DeviceDataset(u8, rows, 0, DEV, spatial_k=24).batches(13, prefetch=False)))
    for key in ("images", "bboxes", "labels", "context_indices"):
        assert torch.equal(a[key], b[key]), key
    assert next(iter(ds.batches(13, prefetch=False)))["context_indices"].shape[1] == 24      # the window of 12, as before
    with pytest.raises(ValueError, match="spatial_k"):
        ds.with_context(spatial_k=-1)


# ---------------------------------------------------------------- 4. the default is untouched
def test_spatial_k_zero_is_the_path_without_the_argument():
    u8, rows = small_dataset()
    plain, zero = DeviceDataset(u8, rows, 4, DEV), DeviceDataset(u8, rows, 4, DEV, spatial_k=0)
    for sf in (1.0, 0.9):
        kw = dict(batch_size=5, shuffle=True, sampling_fraction=sf, seed=2, epoch=3, prefetch=False)
        a, la = profiled(lambda: epoch_tensors(plain, **kw))
        b, lb = profiled(lambda: epoch_tensors(zero, **kw))
        assert la == lb and "cova_context_knn" not in lb and lb["cova_collate_selected"] == 3
        for x, y in zip(a, b):
            for key in ("images", "bboxes", "labels", "context_indices", "additional_feats", "page_start"):
                assert torch.equal(x[key], y[key]), key
    ids = [3, 0, 7]
    c, lc = profiled(lambda: DeviceCollate(4, DEV, spatial_k=0)(u8[ids], [rows[i] for i in ids]))
    d, ld = profiled(lambda: DeviceCollate(4, DEV)(u8[ids], [rows[i] for i in ids]))
    assert lc == ld == {"cova_images_u8_to_f32": 1, "cova_collate_boxes": 1}
    for key in ("images", "bboxes", "labels", "context_indices", "additional_feats", "page_start"):
        assert torch.equal(c[key], d[key]), key
    # and a spatial dataset issues the graph launch once per batch, behind a collation that writes no window
    _, ls = profiled(lambda: epoch_tensors(zero.with_context(spatial_k=6), batch_size=5, prefetch=False))
    assert ls["cova_context_knn"] == 3 and ls["cova_collate_selected"] == 3


# ---------------------------------------------------------------- 5. through the model
def test_five_train_steps_on_the_device_graph_equal_steps_on_the_oracle_graph_bit_for_bit():
    u8, rows = page_set()
    sd = seeded(CFG)
    cs, k, bs, sf, seed, epoch = 0, 8, 3, 0.9, 12, 0
    ds = DeviceDataset(u8, rows, cs, DEV, spatial_k=k)
    a, b = HotPathTrainer(CFG, sd, DEV), HotPathTrainer(CFG, sd, DEV)
    losses_a, losses_b = [], []
    for batch in ds.batches(bs, shuffle=True, sampling_fraction=sf, seed=seed, epoch=epoch):
        assert batch["context_indices"].shape[1] == k
        losses_a.append(a.train_step(batch)[0])
    for ids in pipeline.epoch_plan(len(ds), bs, True, seed, epoch):
        host = DeviceCollate(cs, DEV, sampling_fraction=sf, seed=seed)(u8[ids], [rows[i] for i in ids], page_ids=ids, epoch=epoch)
        assert host["context_indices"].numel() == 0
        host["context_indices"] = torch.from_numpy(
            GO.batch_graph(host["bboxes"].cpu().numpy(), host["page_start"].cpu().numpy(), cs, k)).to(DEV)
        losses_b.append(b.train_step(host)[0])
    assert len(losses_a) == len(losses_b) == 5
    assert [float(x) for x in losses_a] == [float(x) for x in losses_b] and all(np.isfinite(float(x)) for x in losses_a)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert not torch.equal(sa["convnet.0.weight"], sd["convnet.0.weight"].to(DEV))          # the steps did train


def test_gat_layer_on_the_tie_grid_hub_matches_the_oracle():
    """One forward / backward of the GAT layer over the device-built tie-grid graph: box 130 is named by 130 rows, so the
    backward's transposed-CSR row of that node is longer than a wave.  The comparison and its constants are those of
    tests/test_model_gpu.py::test_gat_layer_matches_reference_fixture (gat_layer_k100.npz: Fd = 24, D = 8; 1e-5 of the
    output scale forward, 1e-4 of each gradient's scale backward), with oracle/cova_oracle.py as the reference."""
    bb, ps, cs, k, ref_ctx = kernel_case("tie_grid")
    ctx = torch.from_numpy(run_knn(bb, ps, cs, k)).to(DEV)
    assert int(np.bincount(ref_ctx[ref_ctx >= 0], minlength=131)[130]) == 130 and torch.equal(ctx.cpu(), torch.from_numpy(ref_ctx))
    N, Fd, D = 131, 24, 8
    rs = np.random.RandomState(11)
    torch.manual_seed(11)
    layer = GraphAttentionLayer(Fd, D)
    sd = {"gat." + key: v.detach().clone().requires_grad_(True) for key, v in layer.state_dict().items()}
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32))
    layer = layer.to(DEV)
    h = h_host.to(DEV).requires_grad_(True)
    hp, attn = layer(h, ctx, return_attn_wts=True)
    (hp * g_host.to(DEV)).sum().backward()
    h_ref = h_host.clone().requires_grad_(True)
    hp_ref, attn_ref = O.gat(h_ref, torch.from_numpy(ref_ctx), sd, return_attn_wts=True)
    (hp_ref * g_host).sum().backward()
    assert relerr(hp.detach().cpu(), hp_ref.detach()) < 1e-5
    assert relerr(attn.cpu(), attn_ref.detach()) < 1e-5
    assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
    for key, p in layer.named_parameters():
        assert relerr(p.grad.cpu(), sd["gat." + key].grad) < 1e-4, key


def test_evaluate_split_and_fit_run_on_a_spatial_dataset():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    tr = HotPathTrainer(CFG, seeded(CFG), DEV, track_metrics=True)             # fit reads the epoch's loss from the metrics
    rep = evaluate_split(tr, val, with_loss=True)
    assert rep.evaluated.all() and rep.ranks.shape == (11, 3) and (rep.ranks >= 0).all() and np.isfinite(rep.loss)
    # the same split, host-fed with the oracle's graph: the same ranks
    batch = next(iter(val.with_context(2, 0).batches(11, prefetch=False)))
    batch["context_indices"] = torch.from_numpy(
        GO.batch_graph(batch["bboxes"].cpu().numpy(), batch["page_start"].cpu().numpy(), 2, 6)).to(DEV)
    whole = next(iter(val.batches(11, prefetch=False)))
    assert torch.equal(whole["context_indices"], batch["context_indices"])
    assert torch.equal(tr.predict(whole)[0], tr.predict(batch)[0])
    out = fit(tr, train, val, 2, 3, sampling_fraction=0.9, seed=12, eval_interval=1)
    assert len(out.history) == 2 and all(h["eval_acc"] is not None and h["boxes"] > 0 for h in out.history)
    assert tr.step_count == 6


def test_one_feature_cache_serves_two_graphs(monkeypatch):
    u8, rows = page_set(P=6, seed=4)
    ds = DeviceDataset(u8, rows, 12, DEV)
    tr = HotPathTrainer(CFG, seeded(CFG), DEV, frozen=("convnet.",), bn_eval=("convnet.",))
    cache = FeatureCache.build(tr, ds)
    cache.check(tr, ds)
    sib = ds.with_context(0, 24)
    cache.check(tr, sib)
    n_vis = engine.backbone_feat(CFG)
    seen = []
    orig = engine.decoder_fwd
    n = 0
    for cached, full in zip(sib.batches(4, features=cache), sib.batches(4, prefetch=False)):
        table, ids = cached["visual_feats"]
        assert table is cache.table and "images" not in cached
        assert cached["context_indices"].shape == (cached["bboxes"].shape[0], 24)
        assert torch.equal(cached["context_indices"], full["context_indices"])
        monkeypatch.setattr(engine, "decoder_fwd", lambda comb, *a, **kw: seen.append(comb[:, :n_vis].clone()) or orig(comb, *a, **kw))
        engine.model_fwd(CFG, tr.params, tr.buffers, full["images"], full["bboxes"], full["additional_feats"],
                         full["context_indices"], False, save=False)
        monkeypatch.setattr(engine, "decoder_fwd", orig)
        assert torch.equal(table[ids.long()], seen[-1]) and float(seen[-1].abs().max()) > 0      # rows bit-equal to recomputing
        assert torch.equal(tr.predict(cached)[0], tr.predict(full)[0])
        n += 1
    assert n == 2
    # the two graphs differ, the cache does not care
    a = next(iter(ds.batches(6, features=cache)))
    b = next(iter(sib.batches(6, features=cache)))
    assert torch.equal(a["visual_feats"][1], b["visual_feats"][1]) and not torch.equal(a["context_indices"], b["context_indices"])
    loss, _ = tr.train_step(b)
    assert np.isfinite(float(loss))
