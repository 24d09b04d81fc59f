"""Host side of the edge-geometry extension (no GPU): the numpy feature oracle (tests/edge_oracle.py) against a brute-force
loop over np.float32 scalars, the torch layer oracle with a zero edge weight against the plain oracle, and the parameter
list (weights.state_dict_spec) with the option off and on."""
import numpy as np
import pytest
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, weights

import edge_oracle as EO
from oracle import cova_oracle as O
from config_cases import SPLIT_CFG  # noqa: E402


def brute_force(bboxes, ctx, img_w, img_h):
    """The contract in Python scalars: one np.float32 operation per rounding."""
    f = np.float32
    b = [[f(v) for v in row[1:]] for row in np.asarray(bboxes, dtype=np.float32)]
    N, K = ctx.shape
    W, H = f(img_w), f(img_h)
    out = np.zeros((N, K, 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(N):
            for k in range(K):
                j = int(ctx[i, k])
                if j < 0 or j >= N:
                    continue
                (x1i, y1i, x2i, y2i), (x1j, y1j, x2j, y2j) = b[i], b[j]
                wi, hi, wj, hj = f(x2i - x1i), f(y2i - y1i), f(x2j - x1j), f(y2j - y1j)
                p = out[i, k]
                p[0] = f(f(f(x1j + x2j) - f(x1i + x2i)) / f(f(2) * W))
                p[1] = f(f(f(y1j + y2j) - f(y1i + y2i)) / f(f(2) * H))
                p[2] = f(f(wj - wi) / f(f(wj + wi) + f(1)))
                p[3] = f(f(hj - hi) / f(f(hj + hi) + f(1)))
                p[4] = f(max(f(0), f(max(x1i, x1j) - min(x2i, x2j))) / W)
                p[5] = f(max(f(0), f(max(y1i, y1j) - min(y2i, y2j))) / H)
                iw = max(f(0), f(min(x2i, x2j) - max(x1i, x1j)))
                ih = max(f(0), f(min(y2i, y2j) - max(y1i, y1j)))
                inter = f(iw * ih)
                uni = f(f(f(wi * hi) + f(wj * hj)) - inter)
                p[6] = f(inter / uni) if uni > 0 else f(0)
                p[7] = f(f(max(-64, min(64, j - i))) / f(64))
    return out


def boxes_case(rs, n, half_pixel):
    wh = rs.randint(1, 300, (n, 2)).astype(np.float32)
    xy = rs.randint(0, 900, (n, 2)).astype(np.float32)
    if half_pixel:
        wh, xy = wh + np.float32(0.5) * rs.randint(0, 2, (n, 2)), xy + np.float32(0.5) * rs.randint(0, 2, (n, 2))
    bb = np.zeros((n, 5), np.float32)
    bb[:, 1:3], bb[:, 3:] = xy, (xy + wh).astype(np.float32)
    return bb


def test_numpy_features_equal_the_scalar_statement():
    rs = np.random.RandomState(5)
    for half in (False, True):
        bb = boxes_case(rs, 90, half)
        bb[7] = bb[3]                                  # identical boxes: IoU 1, everything else 0
        bb[11, 3:] = bb[11, 1:3]                       # zero-area boxes (a point) ...
        bb[12] = bb[11]                                # ... twice at one place: uni == 0
        bb[13, 3] = bb[13, 1]                          # zero width, some height
        ctx = rs.randint(-1, 90, (90, 9)).astype(np.int64)
        ctx[3, 0], ctx[7, 0], ctx[11, 0], ctx[12, 0], ctx[11, 1], ctx[13, 0] = 7, 3, 12, 11, 11, 13
        ctx[5] = -1                                    # an all-pad row
        ctx[6, 2] = 90                                 # an id >= N: a pad
        ctx[0, 3], ctx[89, 3] = 89, 0                  # |j - i| > 64: the clamp of phi7
        got = EO.edge_features(bb, ctx, 1280, 960)
        ref = brute_force(bb, ctx, 1280, 960)
        assert got.dtype == np.float32 and got.shape == (90, 9, 8)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        assert not got[5].any() and not got[6, 2].any()
        assert got[3, 0, 6] == 1.0 and not got[3, 0, :6].any() and got[3, 0, 7] == np.float32(4 / 64)
        assert got[11, 0, 6] == 0.0 and got[12, 0, 6] == 0.0 and got[11, 1, 6] == 0.0        # uni == 0 -> 0, not NaN
        assert got[0, 3, 7] == 1.0 and got[89, 3, 7] == -1.0
        assert np.isfinite(got).all()
    assert EO.edge_features(np.zeros((0, 5), np.float32), np.zeros((0, 4), np.int64), 10, 10).shape == (0, 4, 8)


def test_features_are_antisymmetric_or_symmetric_as_stated():
    rs = np.random.RandomState(9)
    bb = boxes_case(rs, 40, True)
    ctx = np.stack([np.roll(np.arange(40), 1), np.roll(np.arange(40), -3)], 1).astype(np.int64)
    phi = EO.edge_features(bb, ctx, 1280, 1280)
    back = np.zeros_like(phi)
    for i in range(40):
        for k in range(2):
            j = ctx[i, k]
            rev = np.array([[i]], np.int64)
            full = np.full((40, 1), -1, np.int64)
            full[j] = rev
            back[i, k] = EO.edge_features(bb, full, 1280, 1280)[j, 0]
    assert np.array_equal(back[..., [0, 1, 2, 3, 7]], -phi[..., [0, 1, 2, 3, 7]])            # offsets and contrasts flip sign
    assert np.array_equal(back[..., 4:7], phi[..., 4:7])                                     # gap and IoU do not


def layer_case(seed, N=23, Fd=19, D=12, K=7):
    rs = np.random.RandomState(seed)
    sd = {"gat.W_i.weight": torch.from_numpy(rs.standard_normal((D, Fd)).astype(np.float32)),
          "gat.W_j.weight": torch.from_numpy(rs.standard_normal((D, Fd)).astype(np.float32)),
          "gat.attention_layer.weight": torch.from_numpy(rs.standard_normal((1, 2 * D)).astype(np.float32)),
          "gat.attention_layer.bias": torch.from_numpy(rs.standard_normal(1).astype(np.float32)),
          "gat.edge_layer.weight": torch.zeros(1, 8)}
    h = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    ctx = torch.from_numpy(rs.randint(-1, N, (N, K)).astype(np.int64))
    ctx[2] = -1
    bb = boxes_case(rs, N, True)
    phi = torch.from_numpy(EO.edge_features(bb, ctx.numpy(), 1280, 1280))
    return sd, h, ctx, bb, phi


def test_torch_layer_with_a_zero_edge_weight_is_the_plain_oracle():
    sd, h, ctx, bb, phi = layer_case(3)
    hp, attn = EO.gat(h, ctx, sd, phi, return_attn_wts=True)
    hp_ref, attn_ref = O.gat(h, ctx, sd, return_attn_wts=True)
    assert torch.equal(hp, hp_ref) and torch.equal(attn, attn_ref)
    sd["gat.edge_layer.weight"] = torch.linspace(-2, 2, 8).view(1, 8)
    hp2, attn2 = EO.gat(h, ctx, sd, phi, return_attn_wts=True)
    assert not torch.equal(attn2, attn_ref)                        # the term is live ...
    assert torch.equal(attn2[2], attn_ref[2]) and float(hp2[2].abs().max()) == 0.0          # ... but not on an all-pad row
    patched = EO.patched_gat(torch.from_numpy(bb), (1280, 1280))
    assert torch.equal(patched(h, ctx, sd, 0.2, True)[1], attn2)
    plain_sd = {k: v for k, v in sd.items() if "edge_layer" not in k}
    assert torch.equal(patched(h, ctx, plain_sd, 0.2, True)[1], attn_ref)


def test_default_spec_is_unchanged_and_the_option_adds_one_key_per_head():
    base = weights.state_dict_spec()
    assert len(base) == 50 and base == weights.state_dict_spec(edge_geometry=False)
    assert not any("edge_layer" in k for k, _ in base)
    on = weights.state_dict_spec(edge_geometry=True)
    assert [e for e in on if e not in base] == [("gat.edge_layer.weight", (1, 8))]
    assert [e for e in on if "edge_layer" not in e[0]] == base
    keys = [k for k, _ in on]
    at = keys.index("gat.edge_layer.weight")
    assert keys[at - 4:at] == ["gat.W_i.weight", "gat.W_j.weight", "gat.attention_layer.weight", "gat.attention_layer.bias"]
    base22 = weights.state_dict_spec(n_heads=2, n_gat_layers=2)
    on22 = weights.state_dict_spec(n_heads=2, n_gat_layers=2, edge_geometry=True)
    assert [e for e in on22 if e not in base22] == [("gat.layers.%d.heads.%d.edge_layer.weight" % (l, h), (1, 8))
                                                    for l in range(2) for h in range(2)]
    assert [e for e in on22 if "edge_layer" not in e[0]] == base22
    assert weights.state_dict_spec(use_context=False, edge_geometry=True) == weights.state_dict_spec(use_context=False)


def test_seeded_weights_start_the_edge_term_at_zero_and_leave_the_rest_alone():
    plain = weights.seeded_state_dict(7, n_heads=2, n_gat_layers=2)
    edge = weights.seeded_state_dict(7, n_heads=2, n_gat_layers=2, edge_geometry=True)
    extra = [k for k in edge if k not in plain]
    assert len(extra) == 4 and all(k.endswith("edge_layer.weight") and not edge[k].any() for k in extra)
    assert all(torch.equal(edge[k], plain[k]) for k in plain)


def test_header_declares_the_edge_entry_points():
    protos = _lib.parse_header()
    assert len(protos["cova_edge_geometry"]) == 8                                  # (the stream included)
    assert len(protos["cova_gat_fwd_edge"]) == len(protos["cova_gat_fwd"]) + 2     # phi, edge_w
    assert len(protos["cova_gat_bwd_edge"]) == len(protos["cova_gat_bwd"]) + 4     # phi, edge_w, d_edge_w, workspace
    assert len(protos["cova_gat_edge_workspace_floats"]) == 2


# ---------------------------------------------------------------- the trainer's host side (flat buckets, groups, checkpoints)
from cova_web_object_detection_amd import engine  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

TCFG = dict(SPLIT_CFG, n_heads=2, n_gat_layers=2, edge_geometry=True)
TSD = weights.seeded_state_dict(5, **{k: v for k, v in TCFG.items() if k != "drop_prob"})
EDGE_KEYS = [k for k in TSD if k.endswith("edge_layer.weight")]


def test_trainer_buckets_groups_and_frozen_sets_take_the_edge_weights_from_the_spec():
    tr = HotPathTrainer(TCFG, TSD, "cpu")
    assert len(EDGE_KEYS) == 4 and all(k in tr.params and tr.grads[k].shape == (1, 8) for k in EDGE_KEYS)
    head = tr._head_offset()
    for k in EDGE_KEYS:                                    # in the head range of the two-phase gradient all-reduce
        assert tr.gbucket.offsets[k][0] >= head and tr.gbucket.offsets[k][0] % 4 == 0
        p = k[:-len("edge_layer.weight")]
        assert engine._adjacent(tr.params[p + "W_i.weight"], tr.params[p + "W_j.weight"])      # one-GEMM projections kept
        assert engine._adjacent(tr.grads[p + "W_i.weight"], tr.grads[p + "W_j.weight"])
    assert tr.plan is None and tr._adam_runs == [(0, tr.pbucket.flat.numel())]
    grouped = HotPathTrainer(TCFG, TSD, "cpu", optimizer="adamw",
                             param_groups=[dict(params=[k[:-len("weight")] for k in EDGE_KEYS], lr=1e-2, weight_decay=0.0)])
    assert grouped.param_groups[0]["params"] == EDGE_KEYS and not set(EDGE_KEYS) & set(grouped.param_groups[1]["params"])
    covered = sum(hi - lo for lo, hi, gid in grouped.optim_runs if gid == 0)
    assert covered == 4 * 8                                # eight floats per head, no padding claimed from a neighbour
    frozen = HotPathTrainer(TCFG, TSD, "cpu", frozen=("gat.layers.0.heads.1.edge_layer.",))
    assert frozen.frozen == {"gat.layers.0.heads.1.edge_layer.weight"}
    lo = frozen.pbucket.offsets["gat.layers.0.heads.1.edge_layer.weight"][0]
    assert not any(a <= lo < b for a, b in frozen._adam_runs) and frozen.plan == engine.full_plan(frozen.params)
    with pytest.raises(KeyError):                          # a plain checkpoint lacks the key: said, not guessed
        tr.load_state_dict({k: v for k, v in TSD.items() if k not in EDGE_KEYS})
    sd = dict(TSD)
    for i, k in enumerate(EDGE_KEYS):
        sd[k] = torch.full((1, 8), float(i + 1))
    tr.load_state_dict(sd)
    back = tr.state_dict()
    assert sorted(back) == sorted(TSD) and all(torch.equal(back[k], sd[k]) for k in sd)
    other = HotPathTrainer(TCFG, TSD, "cpu")
    other.load_optimizer_state_dict(tr.optimizer_state_dict())
    assert other.exp_avg.numel() == tr.pbucket.flat.numel()
    with pytest.raises(ValueError):                        # moments of a plain trainer do not fit
        plain = {k: v for k, v in TCFG.items() if k != "edge_geometry"}
        HotPathTrainer(plain, TSD, "cpu").load_optimizer_state_dict(tr.optimizer_state_dict())


def test_gradient_allreduce_ranges_cover_the_edge_weights(tmp_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "store"), rank=0, world_size=1)
    try:
        tr = HotPathTrainer(TCFG, TSD, "cpu", world_size=1)
        tr.gbucket.flat.fill_(1.0)
        n, head = tr.gbucket.flat.numel(), tr._head_offset()
        tr.gbucket.all_reduce_range(head, n)               # the head phase (trainer._reduce_head) ...
        tr.gbucket.all_reduce_range(0, head)               # ... and the conv-stack phase: together the whole bucket, once
        assert all(bool((tr.grads[k] == 1.0).all()) for k in EDGE_KEYS)
        spans = sorted((o, o + m) for o, m, _ in tr.gbucket.offsets.values())
        assert spans[0][0] == 0 and spans[-1][1] <= n and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    finally:
        dist.destroy_process_group()
