"""N > 1 path on CPU (gloo, world_size 2): page sharding, the flat gradient bucket and its single
all-reduce.  The HIP kernels cannot run here, so each rank's local gradients come from the CPU
oracle (test infrastructure); what is under test is the host logic of trainer.py that the GPU
path uses unchanged (FlatBucket, shard_batch, all_reduce_sum)."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import cova_amd  # noqa: E402,F401  (spawned workers re-import this module without conftest.py)

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cova_web_object_detection_amd import synthetic, weights
from cova_web_object_detection_amd.trainer import FlatBucket, is_param_key, shard_batch, shard_pages
from oracle import cova_oracle as O
from config_cases import DDP_CFG as CFG
from helpers import free_port


def _local_grads(batch):
    wcfg = {k: v for k, v in CFG.items() if k != "drop_prob"}
    sd = weights.seeded_state_dict(9, **wcfg)
    _, _, grads, _, _ = O.loss_and_grads(sd, batch["images"], batch["bboxes"], batch["additional_feats"],
                                         batch["context_indices"], batch["labels"], CFG, None)
    return sd, grads


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    full = synthetic.make_batch(4, img_h=64, boxes_per_page=[11, 20, 15, 30], context_size=4, seed=9)
    shard = shard_batch(full, rank, world)
    sd, grads = _local_grads(shard)
    bucket = FlatBucket({k: tuple(v.shape) for k, v in sd.items() if is_param_key(k)}, "cpu")
    for k, g in grads.items():
        bucket.views[k].copy_(g)
    # the trainer's two-phase exchange (head asynchronously first, conv stack at the end) on a copy
    two = FlatBucket({k: tuple(v.shape) for k, v in sd.items() if is_param_key(k)}, "cpu")
    two.flat.copy_(bucket.flat)
    lo = two.split_at("bbox_feat_encoder.0.weight")
    work = two.all_reduce_range(lo, two.flat.numel(), async_op=True)
    two.all_reduce_range(0, lo)
    work.wait()
    bucket.all_reduce_sum()
    assert torch.equal(two.flat, bucket.flat), "two-phase all-reduce differs from the single collective"
    torch.save({k: v.clone() for k, v in bucket.views.items()}, os.path.join(out_dir, "r%d.pt" % rank))
    dist.destroy_process_group()


def test_shard_pages_and_rebase():
    assert [shard_pages(5, r, 2) for r in range(2)] == [(0, 3), (3, 5)]
    assert [shard_pages(16, r, 8) for r in range(8)] == [(2 * r, 2 * r + 2) for r in range(8)]
    full = synthetic.make_batch(4, img_h=32, boxes_per_page=[11, 20, 15, 30], context_size=4, seed=3)
    s1 = shard_batch(full, 1, 2)
    assert s1["images"].shape[0] == 2 and s1["bboxes"].shape[0] == 45
    assert set(s1["bboxes"][:, 0].tolist()) == {0.0, 1.0}
    ref = synthetic.collate_context([synthetic.context_window_indices(n, 4) for n in (15, 30)])
    assert np.array_equal(s1["context_indices"].numpy(), ref)
    assert torch.equal(s1["labels"], full["labels"][31:])


def test_flat_bucket_views_alias_one_buffer():
    shapes = {"a": (3, 5), "b": (7,), "c": (2, 2, 2)}
    b = FlatBucket(shapes, "cpu")
    b.views["b"].fill_(2.0)
    assert b.flat.sum().item() == 14.0 and b.flat.numel() % 4 == 0
    assert all(v.data_ptr() % 16 == 0 for v in b.views.values())


@pytest.mark.timeout(300)
def test_gloo_allreduce_of_flat_bucket_equals_sum_of_shard_gradients(tmp_path):
    world, port = 2, free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    full = synthetic.make_batch(4, img_h=64, boxes_per_page=[11, 20, 15, 30], context_size=4, seed=9)
    expect = None
    for r in range(world):
        _, g = _local_grads(shard_batch(full, r, world))
        expect = g if expect is None else {k: expect[k] + g[k] for k in g}
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "r%d.pt" % r)) for r in range(world))
    for k, v in expect.items():
        assert torch.equal(r0[k], r1[k]), k                       # every rank holds the same sum
        assert torch.allclose(r0[k], v, rtol=1e-4, atol=1e-4 * max(1.0, float(v.abs().max()))), k  # thread-count dependent summation order


def _state_worker(rank, world, port, out_dir):
    """load_state_dict / load_optimizer_state_dict of HotPathTrainer across two ranks (flat buckets on the CPU: no device work)."""
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    wcfg = {k: v for k, v in CFG.items() if k != "drop_prob"}
    res = {}
    tr = HotPathTrainer(CFG, weights.seeded_state_dict(40 + rank, **wcfg), "cpu", world_size=world)
    res["start"] = tr.pbucket.flat.clone()                       # rank 0's weights everywhere (start-up broadcast)
    # a rank-0-only reload (train.py:94 "reload best" on one rank) is LOCAL: no collective, no hang
    if rank == 0:
        tr.load_state_dict(weights.seeded_state_dict(77, **wcfg))
    res["after_local"] = tr.pbucket.flat.clone()
    # broadcast=True: parameters and buffers of rank 0 everywhere, the Adam moments and step count stay this rank's
    tr.exp_avg.fill_(float(rank + 1))
    tr.step_count = 10 + rank
    tr.load_state_dict(weights.seeded_state_dict(50 + rank, **wcfg), broadcast=True)
    res["after_bcast"] = tr.pbucket.flat.clone()
    res["moments_kept"] = bool((tr.exp_avg == float(rank + 1)).all()) and tr.step_count == 10 + rank
    # a state_dict that only ONE rank cannot validate raises on BOTH (nobody is left inside the broadcast)
    bad = weights.seeded_state_dict(60, **wcfg)
    if rank == 1:
        bad = {"convnet.0.weight": bad["convnet.0.weight"]}
    try:
        tr.load_state_dict(bad, broadcast=True)
        res["raised"] = False
    except KeyError:
        res["raised"] = True
    res["unchanged_after_error"] = torch.equal(tr.pbucket.flat, res["after_bcast"]) if rank == 1 else True
    # optimizer state: moments, step count and hyper-parameters of rank 0
    st = tr.optimizer_state_dict()
    st["hp"]["lr"] = 1e-3 * (rank + 1)
    tr.load_optimizer_state_dict(st, broadcast=True)
    res["opt"] = (tr.step_count, tr.hp["lr"], float(tr.exp_avg[0]))
    torch.save(res, os.path.join(out_dir, "s%d.pt" % rank))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_trainer_state_loads_are_local_unless_broadcast_is_asked_for(tmp_path):
    """load_state_dict / load_optimizer_state_dict involve a collective only with broadcast=True; then keys are
    validated on every rank before the broadcast, which carries what was loaded and nothing else."""
    world, port = 2, free_port()
    mp.spawn(_state_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "s%d.pt" % r)) for r in range(world))
    assert torch.equal(r0["start"], r1["start"])
    assert not torch.equal(r0["after_local"], r1["after_local"]) and torch.equal(r1["after_local"], r1["start"])
    assert torch.equal(r0["after_bcast"], r1["after_bcast"]) and not torch.equal(r0["after_bcast"], r0["after_local"])
    assert r0["moments_kept"] and r1["moments_kept"]
    assert r0["raised"] and r1["raised"] and r1["unchanged_after_error"]
    assert r0["opt"] == r1["opt"] == (10, 1e-3, 1.0)
