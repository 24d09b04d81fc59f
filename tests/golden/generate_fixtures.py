#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own code (dev container only).

    python tests/golden/generate_fixtures.py        # needs /root/reference (read-only)
    python tests/golden/generate_fixtures.py case_cova_cs0 case_cova_roi5_odd     # only these (the others stay byte-identical)

The reference (pure Python) cannot travel to the GPU box, so its outputs are captured here
as data.  ``/root/reference`` is put first on sys.path (its ``datasets.py`` would otherwise be
shadowed by the HuggingFace package of the same name) and the build-owned stand-in for the
missing ``torchvision`` namespace (tests/golden/_standin) second; ``models.CoVA``,
``models.GraphAttentionLayer``, ``datasets.WebDataset/custom_collate_fn`` and
``train.evaluate_model`` then run unmodified.

Fixtures hold inputs (or the seeds that regenerate them through
cova_web_object_detection_amd.synthetic / .weights, both numpy-RandomState based and
platform-stable) and the reference's outputs.  Large gradients are stored as
(norm, strided sample) instead of in full to keep the files small.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_standin"))
sys.path.insert(0, REF)
sys.path.append(ROOT)

import torchvision  # noqa: E402,F401  (the stand-in)
import models as ref_models  # noqa: E402
import datasets as ref_datasets  # noqa: E402
import train as ref_train  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import synthetic, weights  # noqa: E402

assert ref_models.__file__.startswith(REF), ref_models.__file__
assert ref_datasets.__file__.startswith(REF), ref_datasets.__file__

SAMPLE_STRIDE = 97
FULL_LIMIT = 40000


def pack_grad(out, key, g):
    g = g.detach().numpy().astype(np.float32)
    out["gradnorm/" + key] = np.float64(np.linalg.norm(g.astype(np.float64)))
    if g.size <= FULL_LIMIT:
        out["grad/" + key] = g
    else:
        out["gradsample/" + key] = g.reshape(-1)[::SAMPLE_STRIDE].copy()


def build_ref_model(cfg, img_h, sd):
    torch.manual_seed(0)
    m = ref_models.CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"],
                        cfg["hidden_dim"], cfg["bbox_hidden_dim"], cfg["n_additional_feat"],
                        cfg["drop_prob"], None)
    m.load_state_dict(sd)     # also overwrites the BN buffers polluted by models.py:53-54
    return m


def case_full_model(name, n_pages, img_h, boxes, cs, seed, hidden_dim=384, bbox_hidden_dim=32,
                    n_additional_feat=0, logit_gain=8.0, roi=(3, 3), use_context=True):
    cfg = dict(roi_output_size=tuple(roi), n_classes=4, use_context=use_context, hidden_dim=hidden_dim,
               bbox_hidden_dim=bbox_hidden_dim, n_additional_feat=n_additional_feat, drop_prob=0.0)
    wcfg = {k: cfg[k] for k in ("roi_output_size", "n_classes", "use_context", "hidden_dim",
                                "bbox_hidden_dim", "n_additional_feat")}
    sd = weights.seeded_state_dict(seed, logit_gain=logit_gain, **wcfg)
    batch = synthetic.make_batch(n_pages, img_h=img_h, boxes_per_page=boxes, context_size=cs,
                                 n_additional_feat=n_additional_feat, seed=seed)
    out = {"meta/n_pages": n_pages, "meta/img_h": img_h,
           "meta/boxes": np.asarray(boxes if not np.isscalar(boxes) else [boxes] * n_pages),
           "meta/context_size": cs, "meta/seed": seed, "meta/hidden_dim": hidden_dim,
           "meta/bbox_hidden_dim": bbox_hidden_dim, "meta/n_additional_feat": n_additional_feat,
           "meta/logit_gain": logit_gain, "meta/roi_output_size": np.asarray(roi, dtype=np.int64),
           "meta/use_context": np.bool_(use_context)}
    args = (batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"])

    # ---- eval mode (running statistics), the mode predictions are taken in (train.py:112)
    m = build_ref_model(cfg, img_h, sd)
    m.eval()
    with torch.no_grad():
        logits = m(*args)
        visual = m._get_visual_features(batch["images"], batch["bboxes"])
        bbf = m._get_bbox_features(batch["bboxes"])
        own = torch.cat((visual, bbf, m.bn_additional_feat(batch["additional_feats"])), dim=1)
        if use_context:
            hp, attn = m.gat(own, batch["context_indices"], return_attn_wts=True)
            hp, attn = hp.numpy(), attn.numpy()
        else:                          # `--context_size 0` (main.py:58-59): the model has no GAT
            hp, attn = np.zeros((0,), np.float32), np.zeros((0, 0), np.float32)
    out["eval/logits"] = logits.numpy()
    out["eval/visual_sample"] = visual.numpy().reshape(-1)[::7].copy()
    out["eval/bbox_feats"] = bbf.numpy()
    out["eval/attn"] = attn
    out["eval/context_sample"] = hp.reshape(-1)[::5].copy()
    out["eval/argmax"] = logits.argmax(dim=1).numpy()
    dec = []
    for index in torch.unique(batch["bboxes"][:, 0]).long():
        o = logits[batch["bboxes"][:, 0] == index]
        dec.append(torch.argsort(o, dim=0)[o.shape[0] - 1:].numpy()[0])     # train.py:144-146, k=1
    out["eval/page_class_top1"] = np.stack(dec)

    # ---- train mode (batch statistics), Dropout(p=0) == identity: forward, CE-sum, backward
    m = build_ref_model(cfg, img_h, sd)
    ref_sd = m.state_dict()            # names and shapes of the reference's own state_dict: data
    out["meta/state_keys"] = np.asarray(list(ref_sd.keys()))
    out["meta/state_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
    m.train()
    logits = m(*args)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"])   # main.py:139
    loss.backward()
    out["train/logits"] = logits.detach().numpy()
    out["train/loss"] = np.float64(loss.item())
    for k, p in m.named_parameters():
        pack_grad(out, k, p.grad)
    for k, b in m.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["buf/" + k] = b.detach().numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "loss", loss.item(), "bytes", os.path.getsize(os.path.join(HERE, name + ".npz")))


def case_cova_roi1_bare():
    """smallest model: T = n_vis = 64, decoder only, a one-box page"""
    case_full_model("cova_roi1_bare", 2, 64, [13, 1], 0, seed=105, hidden_dim=0, bbox_hidden_dim=0, roi=(1, 1),
                    use_context=False)


def case_cova_cs0():
    """the `-cs 0` ablation (main.py:58-59 passes hidden_dim=0) at the standard widths, T = 608"""
    case_full_model("cova_cs0", 2, 64, [40, 25], 0, seed=106, hidden_dim=0, bbox_hidden_dim=32, use_context=False)


def case_cova_roi2x3_cs1():
    """non-square bins, K = 2"""
    case_full_model("cova_roi2x3_cs1", 2, 64, [30, 9], 1, seed=107, hidden_dim=64, bbox_hidden_dim=16, roi=(2, 3))


def case_cova_roi5_odd():
    """n_vis = 1600, F = 1610, T = 1710: no row of the [N, T] matrix and none of its column blocks (at 1600, 1607,
    1610) starts on a 16-byte boundary"""
    case_full_model("cova_roi5_odd", 3, 128, [11, 70, 2], 3, seed=108, hidden_dim=100, bbox_hidden_dim=7,
                    n_additional_feat=3, roi=(5, 5))


def case_gat(name="gat_layer", seed=7, N=13, K=6, Fd=40, D=16):
    """models.GraphAttentionLayer on hand-made graphs, incl. an all -1 row."""
    rs = np.random.RandomState(seed)
    layer = ref_models.GraphAttentionLayer(Fd, D)
    sd = {"W_i.weight": torch.from_numpy(rs.uniform(-0.3, 0.3, (D, Fd)).astype(np.float32)),
          "W_j.weight": torch.from_numpy(rs.uniform(-0.3, 0.3, (D, Fd)).astype(np.float32)),
          "attention_layer.weight": torch.from_numpy(rs.uniform(-0.5, 0.5, (1, 2 * D)).astype(np.float32)),
          "attention_layer.bias": torch.from_numpy(rs.uniform(-0.5, 0.5, (1,)).astype(np.float32))}
    layer.load_state_dict(sd)
    h = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32)).requires_grad_(True)
    ctx = rs.randint(0, N, (N, K)).astype(np.int64)
    ctx[3, :] = -1                      # isolated node
    ctx[5, 2:] = -1                     # trailing pads
    ctx[8, :] = 8                       # repeated neighbour (API accepts arbitrary indices)
    ctx_t = torch.from_numpy(ctx)
    hp, attn = layer(h, ctx_t, return_attn_wts=True)
    g = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32))
    (hp * g).sum().backward()
    out = {"h": h.detach().numpy(), "ctx": ctx, "g": g.numpy(), "h_prime": hp.detach().numpy(),
           "attn": attn.detach().numpy(), "grad_h": h.grad.numpy()}
    for k, v in sd.items():
        out["w/" + k] = v.numpy()
    for k, p in layer.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "ok")


def case_gat_k100():
    """n_context = 100 (`-cs 50`): more neighbour slots than a wavefront has lanes (models.py:171-177 takes any K)"""
    case_gat("gat_layer_k100", seed=11, N=150, K=100, Fd=24, D=8)


def case_collate():
    """datasets.WebDataset.__getitem__ + custom_collate_fn on a 3-page ragged batch."""
    from PIL import Image
    rs = np.random.RandomState(11)
    counts, cs, H = [5, 30, 11], 12, 32
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(d + "/imgs")
        os.makedirs(d + "/bboxes")
        ids = []
        for p, n in enumerate(counts):
            img = (rs.uniform(0, 255, (H, H, 3))).astype(np.uint8)
            Image.fromarray(img).save("%s/imgs/%d.png" % (d, p))
            xywh = rs.uniform(1, 12, (n, 4)).astype(np.float32)
            lab = np.zeros((n, 1), dtype=np.float32)
            lab[:3, 0] = [1, 2, 3]
            np.savetxt("%s/bboxes/%d.csv" % (d, p), np.concatenate([xywh, lab], 1), delimiter=",",
                       header="x,y,w,h,label", comments="", fmt="%.6f")
            ids.append(str(p))
        ds = ref_datasets.WebDataset(d, ids, cs, False, 1)
        items = [ds[i] for i in range(len(ids))]
        img_ids, images, bboxes, addl, ctx, labels = ref_datasets.custom_collate_fn(items)
    np.savez_compressed(os.path.join(HERE, "collate.npz"), counts=np.asarray(counts),
                        context_size=cs, images=images.numpy(), bboxes=bboxes.numpy(),
                        context_indices=ctx.numpy(), labels=labels.numpy(),
                        additional_feats=addl.numpy())
    print("collate ok", tuple(ctx.shape))


def case_collate_raw():
    """Same as case_collate but the fixture also holds the RAW inputs (uint8 HWC pixels, the
    x,y,w,h,label rows as np.loadtxt returns them), for the device-side input pipeline."""
    from PIL import Image
    rs = np.random.RandomState(12)
    counts, cs, H, W = [7, 40, 2, 13], 5, 24, 36
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(d + "/imgs")
        os.makedirs(d + "/bboxes")
        ids, u8, rows = [], [], []
        for p, n in enumerate(counts):
            img = (rs.uniform(0, 256, (H, W, 3))).astype(np.uint8)
            Image.fromarray(img).save("%s/imgs/%d.png" % (d, p))
            u8.append(img)
            xywh = rs.uniform(1, 12, (n, 4)).astype(np.float32)
            lab = np.zeros((n, 1), dtype=np.float32)
            lab[:min(3, n), 0] = [1, 2, 3][:min(3, n)]
            np.savetxt("%s/bboxes/%d.csv" % (d, p), np.concatenate([xywh, lab], 1), delimiter=",",
                       header="x,y,w,h,label", comments="", fmt="%.6f")
            rows.append(np.loadtxt("%s/bboxes/%d.csv" % (d, p), delimiter=",", skiprows=1,
                                   dtype="float32").reshape(n, 5))          # datasets.py:52-60
            ids.append(str(p))
        ds = ref_datasets.WebDataset(d, ids, cs, False, 1)
        items = [ds[i] for i in range(len(ids))]
        img_ids, images, bboxes, addl, ctx, labels = ref_datasets.custom_collate_fn(items)
    np.savez_compressed(os.path.join(HERE, "collate_raw.npz"), counts=np.asarray(counts),
                        context_size=cs, u8_pages=np.stack(u8), rows=np.concatenate(rows, 0),
                        images=images.numpy(), bboxes=bboxes.numpy(), context_indices=ctx.numpy(),
                        labels=labels.numpy())
    print("collate_raw ok", tuple(images.shape), tuple(ctx.shape))


def case_attn_export():
    """The attention dump of extract_attn_wts_and_visualize.py:104-135 (the statements between the
    batch upload and np.savetxt, executed on the reference model) for the inputs of cova_h64_n11."""
    fx = np.load(os.path.join(HERE, "cova_h64_n11.npz"))
    cfg = dict(roi_output_size=(3, 3), n_classes=4, use_context=True,
               hidden_dim=int(fx["meta/hidden_dim"]), bbox_hidden_dim=int(fx["meta/bbox_hidden_dim"]),
               n_additional_feat=int(fx["meta/n_additional_feat"]), drop_prob=0.0)
    wcfg = {k: cfg[k] for k in ("roi_output_size", "n_classes", "use_context", "hidden_dim",
                                "bbox_hidden_dim", "n_additional_feat")}
    sd = weights.seeded_state_dict(int(fx["meta/seed"]), logit_gain=float(fx["meta/logit_gain"]), **wcfg)
    batch = synthetic.make_batch(int(fx["meta/n_pages"]), img_h=int(fx["meta/img_h"]),
                                 boxes_per_page=[int(b) for b in fx["meta/boxes"]],
                                 context_size=int(fx["meta/context_size"]),
                                 n_additional_feat=cfg["n_additional_feat"], seed=int(fx["meta/seed"]))
    model = build_ref_model(cfg, int(fx["meta/img_h"]), sd)
    model.eval()
    images, bboxes, additional_feats = batch["images"], batch["bboxes"], batch["additional_feats"]
    context_indices, labels = batch["context_indices"], batch["labels"]
    N = bboxes.shape[0]
    with torch.no_grad():
        bbox_coords = bboxes[:, 1:].clone()
        bbox_coords[:, 2:] -= bbox_coords[:, :2]
        bbox_coords_padded = torch.cat((bbox_coords, torch.zeros(4).view(1, -1)), dim=0)
        context_bbox_coords = bbox_coords_padded[context_indices.view(-1)].view(N, -1)
        visual_feats = model._get_visual_features(images, bboxes)
        bbox_feats = model._get_bbox_features(bboxes)
        addl = model.bn_additional_feat(additional_feats)
        own_features = torch.cat((visual_feats, bbox_feats, addl), dim=1)
        _, attention_wts = model.gat(own_features, context_indices, return_attn_wts=True)
    sel = labels > 0
    dump_obj = torch.cat((bbox_coords[sel], labels[sel].float().view(-1, 1), context_bbox_coords[sel],
                          attention_wts[sel]), dim=1).numpy()
    np.savez_compressed(os.path.join(HERE, "attn_export.npz"), rows=dump_obj,
                        source=np.asarray("cova_h64_n11"))
    print("attn_export ok", dump_obj.shape)


def case_evaluate():
    """train.evaluate_model's per-page / per-class decision (train.py:131-154) on fixed logits."""
    rs = np.random.RandomState(5)
    counts = [20, 11, 35]
    batch = synthetic.make_batch(3, img_h=32, boxes_per_page=counts, context_size=2, seed=5)
    logits = torch.from_numpy(rs.standard_normal((sum(counts), 4)).astype(np.float32))

    class Fixed(torch.nn.Module):
        n_classes = 4
        class_names = ["BG", "Price", "Title", "Image"]

        def forward(self, *a):
            return logits

    loader = [(np.array(["0", "1", "2"]), batch["images"], batch["bboxes"],
               batch["additional_feats"], batch["context_indices"], batch["labels"])]
    with tempfile.TemporaryDirectory() as d:
        res = {}
        for k in (1, 3):
            img_acc, class_acc = ref_train.evaluate_model(Fixed(), loader, "cpu", k, "TEST",
                                                          d + "/log.txt")
            res["img_acc_k%d" % k] = img_acc
            res["class_acc_k%d" % k] = class_acc
    np.savez_compressed(os.path.join(HERE, "evaluate.npz"), logits=logits.numpy(),
                        bboxes=batch["bboxes"].numpy(), labels=batch["labels"].numpy(), **res)
    print("evaluate ok")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if len(sys.argv) > 1:           # e.g. `generate_fixtures.py case_collate_raw case_attn_export`
        for name in sys.argv[1:]:
            globals()[name]()
        sys.exit(0)
    case_gat()
    case_gat_k100()
    case_collate()
    case_collate_raw()
    case_attn_export()
    case_evaluate()
    # full model: img_H 64/128 keeps inputs regenerable from seeds and outputs small
    case_full_model("cova_h64_n11", 1, 64, 11, 12, seed=101, hidden_dim=64, bbox_hidden_dim=16)
    case_full_model("cova_h64_n90", 1, 64, 90, 12, seed=102)
    case_full_model("cova_h128_ragged", 3, 128, [11, 230, 47], 12, seed=103, hidden_dim=128)
    case_full_model("cova_h64_addfeat", 2, 64, [40, 25], 4, seed=104, hidden_dim=64,
                    n_additional_feat=6)
    case_cova_roi1_bare()
    case_cova_cs0()
    case_cova_roi2x3_cs1()
    case_cova_roi5_odd()
